"""Training logs on disk: what the reference gets from ``tensorboard_log="logs"`` and its
``TensorboardLogger`` callback (main.py:160-208, tensorboardlogger.py:49-110), written with the
standard library alone.

``ScalarLog(log_dir)`` writes every record twice: as one row of ``progress.csv`` and as one ``Event``
of a TensorBoard event file ``events.out.tfevents.<time>.<host>`` -- TFRecord framing (length, masked
CRC-32C of the length, payload, masked CRC-32C of the payload) around hand-encoded protobuf
``Event { wall_time, step, summary { value { tag, simple_value } } }`` messages, after a leading
``file_version = "brain.Event:2"`` record.  ``write_configs`` writes ``env_train_config.txt`` and
``rl_config.txt`` as main.py:202-206 does.

``record_scalars`` names a ``PPO.learn`` record's entries the way the reference's run names them:
``time/episodes`` and ``episodes/avg_*`` (tensorboardlogger.py:67-108), SB3's ``rollout/*``, ``train/*``
and ``time/*``.  Deviation from the reference, on purpose: every ``episodes/avg_*`` value is the mean
of the terminal step's value over all episodes that ended in the rollout; the reference overwrites its
record at every step with that step's finished episodes, and for two terms
(tensorboardlogger.py:87-88) divides the last env's value by the number of finished envs.
"""
from __future__ import annotations

import csv
import math
import os
import socket
import struct
import time

_CRC_TABLE = None


def crc32c(data: bytes) -> int:
    """CRC-32C (Castagnoli, reflected polynomial 0x82F63B78)."""
    global _CRC_TABLE
    if _CRC_TABLE is None:
        tab = []
        for i in range(256):
            c = i
            for _ in range(8):
                c = (c >> 1) ^ 0x82F63B78 if c & 1 else c >> 1
            tab.append(c)
        _CRC_TABLE = tab
    c = 0xFFFFFFFF
    for b in data:
        c = _CRC_TABLE[(c ^ b) & 0xFF] ^ (c >> 8)
    return c ^ 0xFFFFFFFF


def masked_crc(data: bytes) -> int:
    """TFRecord's masked CRC: rotate right by 15, add 0xA282EAD8."""
    c = crc32c(data)
    return (((c >> 15) | (c << 17)) + 0xA282EAD8) & 0xFFFFFFFF


def tfrecord(payload: bytes) -> bytes:
    head = struct.pack("<Q", len(payload))
    return head + struct.pack("<I", masked_crc(head)) + payload + struct.pack("<I", masked_crc(payload))


def _varint(n: int) -> bytes:
    n &= (1 << 64) - 1  # int64 as its two's complement
    out = bytearray()
    while True:
        b = n & 0x7F
        n >>= 7
        if n:
            out.append(b | 0x80)
        else:
            out.append(b)
            return bytes(out)


def _len_field(field: int, body: bytes) -> bytes:
    return _varint(field << 3 | 2) + _varint(len(body)) + body


def encode_event(wall_time: float, step: int, scalars: dict | None = None, file_version: str | None = None) -> bytes:
    """One ``Event`` message: wall_time (1, double), step (2, int64), file_version (3, string) or
    summary (5) of ``Summary.Value { tag (1, string), simple_value (2, float) }`` entries."""
    ev = b"\x09" + struct.pack("<d", wall_time) + b"\x10" + _varint(int(step))
    if file_version is not None:
        ev += _len_field(3, file_version.encode())
    if scalars:
        summary = b"".join(_len_field(1, _len_field(1, tag.encode()) + b"\x15" + struct.pack("<f", float(val)))
                           for tag, val in scalars.items())
        ev += _len_field(5, summary)
    return ev


# the last six are in a record only when the PPO control path is on (PPOConfig.control)
_TRAIN_KEYS = ("policy_loss", "value_loss", "entropy", "clip_fraction", "approx_kl", "n_minibatches", "early_stop",
               "learning_rate", "clip_range", "clip_range_vf")


def record_scalars(rec: dict, total_episodes: float | None = None) -> dict:
    """A ``PPO.learn`` record under the log's names: ``monitor/<key>`` -> ``<key>`` (``monitor/episodes``
    and ``monitor/skipped`` -> ``rollout/episodes`` / ``rollout/skipped``), the update's statistics ->
    ``train/*``, ``norm/*`` and ``eval/*`` as they are, ``time/fps``, ``time/total_timesteps`` and, with ``total_episodes``, the reference's
    cumulative ``time/episodes``."""
    out = {}
    for k, v in rec.items():
        if k.startswith("monitor/"):
            k = k[len("monitor/"):]
            out[k if "/" in k else "rollout/" + k] = v
        elif k.startswith(("train/", "norm/", "eval/")):
            out[k] = v
        elif k in _TRAIN_KEYS:
            out["train/" + k] = v
    if "monitor/episodes" not in rec and "episodes" in rec:
        out["rollout/episodes"] = rec["episodes"]
        out["rollout/ep_rew_mean"] = rec.get("mean_return", float("nan"))
    if "env_steps_per_s" in rec:
        out["time/fps"] = rec["env_steps_per_s"]
    if "timesteps" in rec:
        out["time/total_timesteps"] = rec["timesteps"]
    if total_episodes is not None:
        out["time/episodes"] = total_episodes
    return out


class ScalarLog:
    """``progress.csv`` + (``tensorboard``) an event file under ``log_dir``.  ``write(scalars, step)``
    appends one row / one event; ``log(record)`` does so for a ``PPO.learn`` record (``PPO.learn``'s
    ``logger``), keeping the cumulative episode count of ``time/episodes``."""

    def __init__(self, log_dir: str, tensorboard: bool = True):
        self.log_dir = str(log_dir)
        os.makedirs(self.log_dir, exist_ok=True)
        self.csv_path = os.path.join(self.log_dir, "progress.csv")
        self._csv = open(self.csv_path, "w", newline="")
        self._fields = None
        self.rows_written = 0
        self.total_episodes = 0.0
        self.event_path = None
        self._ev = None
        if tensorboard:
            now = time.time()
            self.event_path = os.path.join(self.log_dir, f"events.out.tfevents.{int(now)}.{socket.gethostname()}")
            self._ev = open(self.event_path, "wb")
            self._ev.write(tfrecord(encode_event(now, 0, file_version="brain.Event:2")))
            self._ev.flush()

    def write_configs(self, env_config, rl_config) -> None:
        """``env_train_config.txt`` and ``rl_config.txt``: ``str()`` of each, as main.py:202-206."""
        for name, cfg in (("env_train_config.txt", env_config), ("rl_config.txt", rl_config)):
            with open(os.path.join(self.log_dir, name), "w") as f:
                f.write(str(cfg))

    def write(self, scalars: dict, step: int) -> None:
        """One CSV row and one event.  A NaN (the means of a window in which no episode ended) is an
        empty CSV cell and is left out of the event, so a curve simply has no point there."""
        vals = {k: float(v) for k, v in scalars.items()}
        keys = ["step", *vals]
        if self._fields is None:
            self._fields = keys
            csv.writer(self._csv).writerow(keys)
        elif any(k not in self._fields for k in keys):
            # a key not seen before (the first monitored record of a run that began without the
            # monitor): the header grows and the rows written so far are copied under it from the file
            self._fields = self._fields + [k for k in keys if k not in self._fields]
            self._csv.close()
            with open(self.csv_path, newline="") as f:
                old = list(csv.DictReader(f))
            self._csv = open(self.csv_path, "w", newline="")
            w = csv.DictWriter(self._csv, self._fields, restval="")
            w.writeheader()
            w.writerows(old)
        present = {k: v for k, v in vals.items() if v == v}
        csv.DictWriter(self._csv, self._fields, restval="").writerow(dict(present, step=int(step)))
        self._csv.flush()
        self.rows_written += 1
        if self._ev is not None:
            self._ev.write(tfrecord(encode_event(time.time(), step, present)))
            self._ev.flush()

    def log(self, rec: dict) -> None:
        n = rec.get("monitor/episodes", rec.get("episodes", 0.0))
        if n == n and not math.isinf(n):
            self.total_episodes += n
        self.write(record_scalars(rec, self.total_episodes), int(rec.get("timesteps", self.rows_written)))

    __call__ = log

    def close(self) -> None:
        for f in (self._csv, self._ev):
            if f is not None and not f.closed:
                f.close()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()


def read_progress(path: str) -> list:
    """``progress.csv`` back as a list of {key: float} rows (empty cells left out)."""
    with open(path, newline="") as f:
        return [{k: float(v) for k, v in row.items() if v != ""} for row in csv.DictReader(f)]


__all__ = ["ScalarLog", "record_scalars", "read_progress", "crc32c", "masked_crc", "tfrecord", "encode_event"]
