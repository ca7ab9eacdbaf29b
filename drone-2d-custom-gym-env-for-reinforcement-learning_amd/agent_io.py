"""Agent files: a zip laid out like SB3's -- ``policy.pth`` is the policy's state_dict under SB3's
names -- whose other members carry what a resumed run needs (``PPO.save`` / ``PPO.load`` assemble and
apply them).  Every member holds tensors or JSON only (``torch.load(weights_only=True)``)."""
from __future__ import annotations

import io
import json
import os
import zipfile

import numpy as np
import torch

AGENT_FORMAT_VERSION = 1
AGENT_MEMBERS = ("data.json", "policy.pth", "train_state.pth", "env_state.pth", "reward_norm.pth")


def _zip_tensors(z: zipfile.ZipFile, name: str) -> dict:
    return torch.load(io.BytesIO(z.read(name)), map_location="cpu", weights_only=True)


def _to_tensors(x):
    """A checkpoint value with every NumPy array as a tensor (so the member loads weights_only)."""
    if isinstance(x, dict):
        return {k: _to_tensors(v) for k, v in x.items()}
    if isinstance(x, torch.Tensor):
        return x.detach().cpu()
    if isinstance(x, np.ndarray):
        return torch.from_numpy(np.ascontiguousarray(x))
    return x


def _to_arrays(sd: dict) -> dict:
    """An ``env_state.pth`` member as ``Drone2dVecEnv.load_state_dict`` takes it: the nested tables
    (curriculum pool, fresh-curriculum recipes) back as NumPy arrays, the state tensors as they are."""
    return {k: ({kk: (vv.numpy() if isinstance(vv, torch.Tensor) else vv) for kk, vv in v.items()}
                if isinstance(v, dict) else v) for k, v in sd.items()}


def write_agent(path: str, data: dict, members: dict) -> str:
    """``data`` as ``data.json`` and every ``members`` entry (name -> tensors) into the zip ``path``,
    written as ``path + ".part"`` and renamed, so a reader never sees half a file."""
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    tmp = path + ".part"
    with zipfile.ZipFile(tmp, "w", zipfile.ZIP_STORED) as z:
        z.writestr("data.json", json.dumps(data, indent=1))
        for name, obj in members.items():
            buf = io.BytesIO()
            torch.save(obj, buf)
            z.writestr(name, buf.getvalue())
    os.replace(tmp, path)
    return path


def read_agent(path: str) -> tuple:
    """(``data.json``, {member: tensors}) of an agent file of this format version (``env_state.pth`` and
    ``reward_norm.pth`` if it has them)."""
    with zipfile.ZipFile(path) as z:
        data = json.loads(z.read("data.json"))
        if data.get("format_version") != AGENT_FORMAT_VERSION:
            raise ValueError(f"{path}: agent format {data.get('format_version')}, expected {AGENT_FORMAT_VERSION}")
        names = ["policy.pth", "train_state.pth"] + [n for n in ("env_state.pth", "reward_norm.pth") if n in z.namelist()]
        return data, {n: _zip_tensors(z, n) for n in names}
