"""libd2d_gif.so (include/d2d_gif.h) on the CPU, through its host twin: every file is decoded again by a GIF
decoder written here from the GIF89a specification (sub-blocks; variable-width LZW with Clear at any point
and the code-equals-next-entry case; transparency composed over a canvas with disposal 1) and, where Pillow
imports, by Pillow too, frame for frame.  Then real pictures from the renderer's twins, the palettes, the
independence of the streams, the ABI, and the host code under sanitizers."""
import ctypes as C
import io
import os
import subprocess

import numpy as np
import pytest

from conftest import GOLDEN, REPO

try:
    from PIL import Image
except ImportError:  # the Pillow half of every comparison is skipped
    Image = None


@pytest.fixture(scope="module")
def G(d2):
    from drone2d_amd import _build, gif

    _build.build_gif()
    return gif


# ------------------------------------------------------------------------------------------ the decoder
def lzw_decode(data: bytes, m: int, n_px: int):
    """GIF89a appendix F.  Returns (indices uint8 [n_px], Clear codes read); the stream must end with the
    End-of-Information code exactly where the pixels do."""
    clear, eoi = 1 << m, (1 << m) + 1
    width, avail, prev = m + 1, clear + 2, -1
    table = [bytes([i]) for i in range(clear)] + [b"", b""]
    out = bytearray()
    acc = nacc = pos = clears = 0
    ended = False
    while True:
        while nacc < width and pos < len(data):
            acc |= data[pos] << nacc
            nacc += 8
            pos += 1
        if nacc < width:
            break
        code = acc & ((1 << width) - 1)
        acc >>= width
        nacc -= width
        if code == clear:
            del table[clear + 2:]
            width, avail, prev = m + 1, clear + 2, -1
            clears += 1
            continue
        if code == eoi:
            ended = True
            break
        if prev < 0:
            assert code < clear, "the first code after a Clear must be a literal"
            s = table[code]
        else:
            assert code <= avail, f"code {code} beyond the table ({avail})"
            s = table[code] if code < avail else table[prev] + table[prev][:1]
            if avail < 4096:
                table.append(table[prev] + s[:1])
                avail += 1
                if avail == (1 << width) and width < 12:
                    width += 1
        out += s
        prev = code
    assert ended, "no End-of-Information code"
    assert pos == len(data) and acc == 0, "bytes or bits behind the End-of-Information code"
    assert len(out) == n_px, f"{len(out)} pixels decoded, {n_px} expected"
    return np.frombuffer(bytes(out), np.uint8), clears


def parse_gif(b: bytes) -> dict:
    """The file's blocks: screen, global table, loop count, and per frame the extension's and descriptor's
    fields, the LZW data and the data's sub-block lengths."""
    assert b[:6] == b"GIF89a"
    w, h = int.from_bytes(b[6:8], "little"), int.from_bytes(b[8:10], "little")
    flags = b[10]
    assert flags & 0x80, "no global colour table"
    n_tab = 2 << (flags & 7)
    o = 13
    table = np.frombuffer(b[o:o + 3 * n_tab], np.uint8).reshape(n_tab, 3)
    o += 3 * n_tab
    g = {"width": w, "height": h, "table": table, "loop": None, "frames": []}
    gce = None
    while True:
        if b[o] == 0x3B:
            assert o == len(b) - 1, "bytes behind the trailer"
            return g
        if b[o] == 0x21 and b[o + 1] == 0xFF:
            assert b[o + 2] == 11 and b[o + 3:o + 14] == b"NETSCAPE2.0" and b[o + 14] == 3 and b[o + 15] == 1
            g["loop"] = int.from_bytes(b[o + 16:o + 18], "little")
            assert b[o + 18] == 0
            o += 19
        elif b[o] == 0x21 and b[o + 1] == 0xF9:
            assert b[o + 2] == 4 and b[o + 7] == 0
            gce = {"disposal": (b[o + 3] >> 2) & 7, "transparent": b[o + 6] if b[o + 3] & 1 else None,
                   "delay": int.from_bytes(b[o + 4:o + 6], "little")}
            o += 8
        else:
            assert b[o] == 0x2C and gce is not None
            f = dict(gce, left=int.from_bytes(b[o + 1:o + 3], "little"), top=int.from_bytes(b[o + 3:o + 5], "little"),
                     w=int.from_bytes(b[o + 5:o + 7], "little"), h=int.from_bytes(b[o + 7:o + 9], "little"))
            assert b[o + 9] == 0, "local table or interlace"
            f["m"] = b[o + 10]
            start = o - 8
            o += 11
            data, blocks = bytearray(), []
            while b[o]:
                blocks.append(b[o])
                data += b[o + 1:o + 1 + b[o]]
                o += 1 + b[o]
            o += 1
            f["data"], f["blocks"], f["chunk_len"] = bytes(data), blocks, o - start
            g["frames"].append(f)
            gce = None


def decode_gif(b: bytes, with_info: bool = False):
    """RGB frames uint8 [T, H, W, 3]: every image composed over the canvas of its predecessors."""
    g = parse_gif(b)
    canvas = np.zeros((g["height"], g["width"]), np.uint8)
    out = []
    for f in g["frames"]:
        assert f["disposal"] == 1
        assert f["left"] + f["w"] <= g["width"] and f["top"] + f["h"] <= g["height"]
        idx, f["clears"] = lzw_decode(f["data"], f["m"], f["w"] * f["h"])
        idx = idx.reshape(f["h"], f["w"])
        assert int(idx.max()) < len(g["table"])
        view = canvas[f["top"]:f["top"] + f["h"], f["left"]:f["left"] + f["w"]]
        keep = idx == f["transparent"] if f["transparent"] is not None else np.zeros_like(idx, bool)
        view[~keep] = idx[~keep]
        out.append(g["table"][canvas])
    frames = np.stack(out) if out else np.zeros((0, g["height"], g["width"], 3), np.uint8)
    return (frames, g) if with_info else frames


def pillow_frames(b: bytes):
    im = Image.open(io.BytesIO(b))
    out = []
    for t in range(im.n_frames):
        im.seek(t)
        out.append(np.asarray(im.convert("RGB")))
    return np.stack(out)


def round_trip(G, idx, palette, check_pillow=True):
    """Encode the index frames [T, H, W] of one stream under ``palette``; both decoders must give back
    ``palette[idx]`` for every frame, every chunk must fit d2dg_frame_cap.  Returns (parsed file, encoder)."""
    pal = G.Palette(palette)
    frames = pal.colours[idx]
    enc = G.HostEncoder(1, idx.shape[1:], pal)
    for f in frames:
        enc.add(f[None])
    lens = np.array(enc.chunk_lens)[:, 0]
    assert (lens > 0).all() and int(lens.max()) <= G.frame_cap(idx.shape[1:])
    assert (enc.inexact == 0).all()
    b = enc.finish()[0]
    got, g = decode_gif(b, with_info=True)
    assert [f["chunk_len"] for f in g["frames"]] == lens.tolist()
    assert got.shape == frames.shape and (got == frames).all()
    assert g["loop"] == 0 and all(f["m"] == pal.min_code_size and f["delay"] == 3 for f in g["frames"])
    assert len(g["table"]) == 1 << pal.bits and (g["table"][:len(pal)] == pal.colours).all()
    assert g["frames"][0]["transparent"] is None and all(f["transparent"] == len(pal) for f in g["frames"][1:])
    if Image is not None and check_pillow:
        assert (pillow_frames(b) == frames).all()
    return g, enc


def distinct_palette(n, seed=0):
    rng = np.random.default_rng(seed)
    packed = rng.choice(1 << 24, n, replace=False)
    return np.stack([packed >> 16, (packed >> 8) & 255, packed & 255], -1).astype(np.uint8)


# ------------------------------------------------------------------------------------------ the cases
# (index frames [T, H, W] and a palette; tests/test_gpu_gif.py encodes the same ones on the device)
COLOUR_COUNTS = [1, 2, 3, 4, 5, 16, 17, 128, 129, 255]
SUB_BLOCK_DATA = (254, 255, 256, 510, 511)


def case_small(G, h, w):
    rng = np.random.default_rng(h)
    idx = rng.integers(0, 14, (4, h, w)).astype(np.uint8)
    idx[2] = idx[1]
    idx[2, h // 2:, w // 3:] = 3
    return idx, G.Palette.model().colours


def case_boxes():
    """(index frames, palette, the image rectangles (left, top, w, h) they must give)."""
    h, w = 24, 80
    rng = np.random.default_rng(5)
    frames = [rng.integers(0, 5, (h, w)).astype(np.uint8)]
    want = [(0, 0, w, h)]

    def change(top, left, bh, bw):
        f = frames[-1].copy()
        f[top:top + bh, left:left + bw] = (f[top:top + bh, left:left + bw] + 1) % 5
        frames.append(f)
        want.append((left, top, bw, bh))

    for bw in (1, 63, 64, 65):
        change(7, 9, 1, bw)
    frames.append(frames[-1].copy())
    want.append((0, 0, 1, 1))
    change(0, 30, 2, 3)          # the top edge
    change(h - 2, 30, 2, 3)      # the bottom edge
    change(5, 0, 3, 2)           # the left edge
    change(5, w - 2, 3, 2)       # the right edge
    change(h - 1, w - 1, 1, 1)   # the last pixel
    change(0, 0, 1, 1)           # the first
    f = frames[-1].copy()        # two far corners: the box is the whole picture, nearly all of it transparent
    f[0, 0], f[h - 1, w - 1] = (f[0, 0] + 1) % 5, (f[h - 1, w - 1] + 1) % 5
    frames.append(f)
    want.append((0, 0, w, h))
    return np.stack(frames), distinct_palette(5), want


def case_one_colour():
    h, w = 120, 200
    rng = np.random.default_rng(2)
    idx = np.stack([np.full((h, w), 2, np.uint8), rng.integers(0, 3, (h, w)).astype(np.uint8), np.full((h, w), 1, np.uint8)])
    return idx, distinct_palette(3)


def case_colours(n):
    rng = np.random.default_rng(n)
    idx = rng.integers(0, n, (3, 40, 61)).astype(np.uint8)
    idx[1, 10:30] = idx[0, 10:30]
    return idx, distinct_palette(n, seed=n)


def case_noise():
    rng = np.random.default_rng(9)
    idx = rng.integers(0, 255, (2, 512, 512)).astype(np.uint8)
    idx[1, :, :100] = idx[0, :, :100]
    return idx, distinct_palette(255, seed=4)


def case_sub_blocks(G):
    """{data bytes: index frame [1, 9, w]} for every length of SUB_BLOCK_DATA, found by scanning widths and seeds
    with the twin."""
    found = {}
    pal = distinct_palette(6)
    for seed in range(40):
        for w in range(8, 200):
            rng = np.random.default_rng(1000 * seed + w)
            idx = rng.integers(0, 6, (1, 9, w)).astype(np.uint8)
            enc = G.HostEncoder(1, (9, w), pal)
            enc.add(pal[idx[0]][None])
            data = int(enc.chunk_lens[0][0]) - 20
            data -= (data + 255) // 256  # chunk = 20 + data + ceil(data / 255)
            if data in SUB_BLOCK_DATA and data not in found:
                found[data] = idx
        if len(found) == len(SUB_BLOCK_DATA):
            break
    return found, pal


def case_nearest():
    """(one RGB frame [8, 8, 3] with off-palette colours, the palette, the indices it must take)."""
    colours = np.array([[0, 0, 0], [10, 0, 0], [0, 10, 0], [10, 0, 0]], np.uint8)  # (index 3 repeats index 1: never chosen)
    f = np.zeros((8, 8, 3), np.uint8)
    f[0, :5] = [[5, 0, 0], [6, 0, 0], [5, 5, 0], [0, 200, 0], [10, 0, 0]]
    want = np.zeros((8, 8), np.uint8)
    want[0, :5] = [0, 1, 0, 2, 1]
    return f, colours, want


def case_any_colours():
    return np.random.default_rng(21).integers(0, 256, (1, 16, 24, 3)).astype(np.uint8)


def case_streams():
    """(RGB frames [7, 3, 20, 33, 3], the palette, an ``active`` mask [7, 3] that differs per call)."""
    rng = np.random.default_rng(3)
    colours = distinct_palette(9)
    T, K = 7, 3
    idx = rng.integers(0, 9, (T, K, 20, 33)).astype(np.uint8)
    idx[3:] = idx[2]
    idx[3:, :, 4:9, 5:20] = rng.integers(0, 9, (T - 3, K, 5, 15))
    active = np.array([[1, 0, 1], [1, 1, 0], [0, 0, 1], [1, 1, 1], [0, 1, 0], [0, 0, 0], [1, 0, 1]], bool)
    return colours[idx], colours, active


# ------------------------------------------------------------------------------------------ 1. round trip
@pytest.mark.parametrize("h,w", [(8, 8), (37, 53)])
def test_round_trip_small_and_odd(G, h, w):
    """D2DR_MIN_SIZE and an odd size (37 x 53 = 1961 pixels: 64 segments of 31 pixels, the last shorter):
    noise, then partial changes, under the model palette's 14 colours."""
    round_trip(G, *case_small(G, h, w))


def test_round_trip_changed_boxes(G):
    """Changed boxes of 1 x 1, 1 x 63, 1 x 64 and 1 x 65 pixels (with 64 segments: one pixel in one segment
    and 63 empty ones; 63 of length 1; 64 of length 1; lengths 2 ... 2, 1 and empty ones), a frame equal to
    its predecessor (a 1 x 1 transparent image at the origin), boxes touching each edge, and the last pixel."""
    idx, pal, want = case_boxes()
    g, _ = round_trip(G, idx, pal)
    assert [(f["left"], f["top"], f["w"], f["h"]) for f in g["frames"]] == want
    still = g["frames"][5]
    assert still["transparent"] == 5 and lzw_decode(still["data"], still["m"], 1)[0].tolist() == [5]


def test_round_trip_one_colour(G):
    """A frame of one colour (the longest runs: every code one pixel longer than the last), first as a whole
    frame, then as the delta of a noise frame."""
    idx, pal = case_one_colour()
    g, _ = round_trip(G, idx, pal)
    # 64 segments of 375 pixels: about 28 codes of at most 6 bits each
    assert len(g["frames"][0]["data"]) < idx[0].size // 10


@pytest.mark.parametrize("n", COLOUR_COUNTS)
def test_round_trip_colour_counts(G, n):
    """Every minimum code size (2 ... 8), and the counts at which the transparent index makes the table
    double (4 colours need 3 bits, 16 need 5, 128 need 8)."""
    g, enc = round_trip(G, *case_colours(n))
    bits = {1: 1, 2: 2, 3: 2, 4: 3, 5: 3, 16: 5, 17: 5, 128: 8, 129: 8, 255: 8}[n]
    assert len(g["table"]) == 1 << bits and g["frames"][0]["m"] == max(2, bits)
    assert (g["table"][n:] == 0).all()


def test_round_trip_noise_beyond_the_dictionary(G):
    """255-colour noise at 512 x 512: a segment is 4096 pixels, nearly every pixel a code, so every segment
    outgrows the dictionary and writes a Clear inside itself -- at 12 bits, the width the decoder has after
    the entry that the code before it makes it add.  The chunk stays under d2dg_frame_cap."""
    assert G.dict_cap() <= 4096
    g, enc = round_trip(G, *case_noise())
    live = 64
    print(f"mid-segment Clears {enc.mid_clears[0]}, chunk lengths {np.array(enc.chunk_lens)[:, 0].tolist()}, "
          f"bound {G.frame_cap(512)}")
    assert enc.mid_clears[0] >= live                     # both frames' segments, at least one each in the first
    assert g["frames"][0]["clears"] >= 2 * live          # the decoder saw them: 64 leading ones and those inside
    assert len(g["frames"][0]["data"]) > 512 * 512       # incompressible: more than a byte per pixel, under the bound


def test_round_trip_sub_block_boundaries(G):
    """Data of 254, 255 and 256 bytes (one short block; exactly one full block; a full block and one byte),
    and of 510 and 511 (the second block's boundary): found by scanning widths and seeds."""
    found, pal = case_sub_blocks(G)
    assert sorted(found) == sorted(SUB_BLOCK_DATA), sorted(found)
    for data, idx in found.items():
        g, _ = round_trip(G, idx, pal)
        assert len(g["frames"][0]["data"]) == data
        assert g["frames"][0]["blocks"] == [255] * (data // 255) + ([data % 255] if data % 255 else [])


# ------------------------------------------------------------------------------------------ 2. real pictures
@pytest.fixture(scope="module")
def corridor_frames(d2):
    """48 HUD frames (text, arcs, shades, trail) of a corridor flight of the oracle backend under the shipped
    agent, drawn by the renderer's CPU twins at 128 x 128."""
    import torch

    from drone2d_amd import abi, harness, hud
    from drone2d_amd.config import ENV_TEST_CONFIG
    from oracle_backend import OracleVecBackend

    be = OracleVecBackend(1, seed=3, **dict(ENV_TEST_CONFIG, scenario="corridor"))
    pol = harness.MlpActor.from_npz(os.path.join(GOLDEN, "agent_17_90.npz"))
    obs = be.reset(seed=3)
    steps, cap = 47, 8
    poses, count, last = np.zeros((1, cap, 3)), np.zeros(1, np.int32), np.zeros((1, 2))
    st = be.orc.get_state()[0]
    hud.shade_update_host([0], st, None, None, 25.0, poses, count, last)
    trail = np.zeros((1, steps + 1, 2), np.float32)
    trail[0, 0] = st[0:2, 0]
    frames = [hud.render_host(be.scenarios, st, obs.numpy(), None, trail, np.array([1], np.int32), None, (poses, count),
                              size=128)[0]]
    gen = torch.Generator().manual_seed(3)
    for t in range(steps):
        a = pol.act(obs, generator=gen)
        obs, _, term, trunc, info = be.step(a)
        assert not bool(term[0] | trunc[0]), "the flight ended early"
        st = be.orc.get_state()[0]
        hud.shade_update_host([0], st, term.numpy(), trunc.numpy(), 25.0, poses, count, last)
        trail[0, t + 1] = st[0:2, 0]
        frames.append(hud.render_host(be.scenarios, st, obs.numpy(), a.numpy(), trail, np.array([t + 2], np.int32),
                                      info.numpy(), (poses, count), size=128)[0])
    be.close()
    assert info.shape == (1, abi.INFO_DIM) and count[0] >= 2
    return np.stack(frames)


def test_real_pictures(G, corridor_frames):
    """The renderer's pictures hold the model palette's colours only: ``inexact`` stays 0 and the decoded
    frames are the frames."""
    frames = corridor_frames
    pal = G.Palette.model()
    assert len(pal) == 14 and len(G.Palette.scan(frames)) <= 14
    enc = G.HostEncoder(1, 128, pal)
    for f in frames:
        enc.add(f[None])
    assert enc.inexact.tolist() == [0]
    b = enc.finish()[0]
    got, g = decode_gif(b, with_info=True)
    assert (got == frames).all()
    boxes = [f["w"] * f["h"] for f in g["frames"]]
    assert boxes[0] == 128 * 128 and max(boxes[1:]) < 128 * 128  # later frames are sub-rectangles
    if Image is not None:
        assert (pillow_frames(b) == frames).all()
    raw = frames.size
    print(f"{len(frames)} frames of 128 x 128: file {len(b)} bytes, raw RGB T*H*W*3 = {raw} bytes ({raw / len(b):.1f}x)")
    assert len(b) < raw // 20


# ------------------------------------------------------------------------------------------ 3. palettes
def test_palette_scan_nearest_uniform(G):
    rng = np.random.default_rng(1)
    cols = np.array([[0, 0, 255], [0, 1, 0], [1, 0, 0], [0, 0, 0], [255, 255, 255], [0, 1, 0]], np.uint8)
    pal = G.Palette.scan(cols[rng.integers(0, 6, (5, 7))])
    assert pal.colours.tolist() == [[0, 0, 0], [0, 0, 255], [0, 1, 0], [1, 0, 0], [255, 255, 255]]  # by r<<16 | g<<8 | b
    with pytest.raises(ValueError, match="256 distinct"):
        G.Palette.scan(distinct_palette(256))
    assert len(G.Palette.scan(distinct_palette(255))) == 255
    model = G.Palette.model().colours.tolist()
    assert model[:3] == [[243, 243, 243], [0, 0, 0], [0, 0, 255]] and model[11:] == [[205, 222, 250], [170, 195, 235], [150, 0, 0]]
    assert len(set(map(tuple, model))) == 14

    # the nearest rule: squared RGB distance, the lowest index on ties; every such pixel is counted
    f, colours, want = case_nearest()
    pal = G.Palette(colours)
    enc = G.HostEncoder(1, 8, pal)
    enc.add(f[None])
    enc.add(f[None])  # the same off-palette pixels again: unchanged on the canvas, counted again
    assert enc.inexact.tolist() == [8]
    assert (enc.canvas[0] == want).all()
    assert (decode_gif(enc.finish()[0])[0] == pal.colours[want]).all()

    uni = G.Palette.uniform()
    assert len(uni) == 252 and uni.colours[0].tolist() == [0, 0, 0] and uni.colours[-1].tolist() == [255, 255, 255]
    assert uni.colours[1].tolist() == [0, 0, 51] and uni.colours[6].tolist() == [0, 42, 0] and uni.colours[42].tolist() == [51, 0, 0]
    pic = case_any_colours()
    d = ((pic[0][:, :, None, :].astype(np.int64) - uni.colours[None, None].astype(np.int64)) ** 2).sum(-1)
    nearest = uni.colours[d.argmin(-1)]  # argmin: the lowest index on ties
    enc = G.HostEncoder(1, (16, 24), uni)
    enc.add(pic[0][None])
    assert enc.inexact[0] == int((pic[0] != nearest).any(-1).sum())
    assert (decode_gif(enc.finish()[0])[0] == nearest).all()


# ------------------------------------------------------------------------------------------ 4. streams
def test_streams_are_independent(G):
    """K = 3 with an ``active`` mask that differs per call: each stream's file is the file of encoding that
    stream's active frames alone."""
    frames, colours, active = case_streams()
    pal = G.Palette(colours)
    T, K = active.shape
    enc = G.HostEncoder(K, (20, 33), pal)
    for t in range(T):
        enc.add(frames[t], active[t])
    lens = np.array(enc.chunk_lens)
    assert ((lens > 0) == active).all()
    files = enc.finish()
    assert files == G.encode_host(frames, pal, active)
    for k in range(K):
        alone = G.encode_host(frames[active[:, k], k][:, None], pal)[0]
        assert files[k] == alone
        assert (decode_gif(files[k]) == frames[active[:, k], k]).all()
    assert len({len(f) for f in files}) > 1
    # after finish the encoder begins new files: the next frame is a first frame again
    enc.add(frames[0])
    assert enc.finish() == G.encode_host(frames[:1], pal)


# ------------------------------------------------------------------------------------------ 5. the ABI
def test_abi(G):
    from drone2d_amd import _native

    lib = G.load()
    assert lib.d2dg_abi_version() == G.ABI_VERSION == 1
    with pytest.raises(G.GifError, match="ABI version 1, expected 2"):
        _native.bind(G.LIB_PATH, G.SIGNATURES, "d2dg_abi_version", G.ABI_VERSION + 1, G.GifError)
    assert 1024 <= G.dict_cap() <= 4096

    # the bound, as the header derives it
    for h, w in ((8, 8), (37, 53), (256, 256), (2048, 2048)):
        n = h * w
        codes = n + 64 + n // (G.dict_cap() - 258) + 1
        data = (12 * codes + 7) // 8
        assert G.frame_cap((h, w)) == 20 + data + (data + 254) // 255
    assert lib.d2dg_frame_cap(7, 8) == 0 and lib.d2dg_frame_cap(8, 2049) == 0
    with pytest.raises(ValueError):
        G.frame_cap(7)

    pal = np.zeros((256, 3), np.uint8)
    vp = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731

    def encode(k=1, w=8, h=8, n=2, delay=3, cap=None, frames=True):
        f = np.zeros((max(k, 1), h, w, 3), np.uint8)
        canvas, has = np.zeros((max(k, 1), h, w), np.uint8), np.zeros(max(k, 1), np.uint8)
        cap = int(lib.d2dg_frame_cap(8, 8)) if cap is None else cap
        chunk, ln = np.zeros((max(k, 1), min(max(cap, 1), 4096)), np.uint8), np.full(max(k, 1), -1, np.int32)
        rc = lib.d2dg_encode_host(k, w, h, vp(pal), n, vp(f) if frames else None, None, delay, vp(canvas), vp(has),
                                  vp(chunk), cap, vp(ln), None, None)
        return rc, ln

    rc, ln = encode()
    assert rc == G.E_OK and ln[0] > 20
    for kw, msg in ((dict(n=0), "palette of 0 colours"), (dict(n=256), "palette of 256 colours"), (dict(w=7), "7 x 8"),
                    (dict(h=2049, cap=1 << 30), "8 x 2049"), (dict(delay=65536), "delay_cs"), (dict(delay=-1), "delay_cs"),
                    (dict(cap=int(lib.d2dg_frame_cap(8, 8)) - 1), "d2dg_frame_cap"), (dict(k=-1), "negative"),
                    (dict(frames=False), "NULL")):
        rc, ln = encode(**kw)
        assert rc == G.E_ARG and msg in lib.d2dg_last_error().decode(), (kw, lib.d2dg_last_error())
        assert (ln == -1).all()  # nothing written: never a truncated file
    assert encode(k=0)[0] == G.E_OK

    # d2dg_create refuses its arguments before it touches a device: no ctx comes back
    for kw, msg in ((dict(streams=0), "max_streams 0"), (dict(streams=4097), "max_streams 4097"), (dict(w=7), "7 x 64"),
                    (dict(h=2049), "64 x 2049"), (dict(n=0), "palette of 0 colours"), (dict(n=256), "palette of 256 colours"),
                    (dict(palette=None), "palette_rgb is NULL")):
        a = dict(dict(streams=1, w=64, h=64, n=14, palette=vp(pal)), **kw)
        h = C.c_void_p(0xDEAD)
        rc = lib.d2dg_create(0, a["streams"], a["w"], a["h"], a["palette"], a["n"], C.byref(h))
        assert rc == G.E_ARG and msg in lib.d2dg_last_error().decode() and h.value is None, (kw, lib.d2dg_last_error())
    assert lib.d2dg_create(0, 1, 64, 64, vp(pal), 14, None) == G.E_ARG
    assert lib.d2dg_restart(None, None) == G.E_ARG
    assert lib.d2dg_encode(None, 1, 8, 8, None, None, 3, None, 0, None, None, None) == G.E_ARG

    out, n = np.zeros(G.FILE_HEADER_MAX, np.uint8), C.c_int32(0)
    assert lib.d2dg_file_header_host(8, 8, vp(pal), 255, 0, vp(out), len(out), C.byref(n)) == G.E_OK and n.value == 800
    assert lib.d2dg_file_header_host(8, 8, vp(pal), 255, 0, vp(out), 799, C.byref(n)) == G.E_ARG
    assert lib.d2dg_file_header_host(8, 8, vp(pal), 256, 0, vp(out), len(out), C.byref(n)) == G.E_ARG
    assert lib.d2dg_file_header_host(8, 8, vp(pal), 0, 0, vp(out), len(out), C.byref(n)) == G.E_ARG
    assert lib.d2dg_file_header_host(8, 4000, vp(pal), 4, 0, vp(out), len(out), C.byref(n)) == G.E_ARG
    assert lib.d2dg_model_palette(None) == G.E_ARG
    head = G.file_header((37, 53), G.Palette.model(), loop=5)
    assert head[:6] == b"GIF89a" and head[6:10] == bytes([53, 0, 37, 0]) and head[10] == 0xF3 and len(head) == 13 + 48 + 19
    assert head[-3:-1] == bytes([5, 0]) and len(G.file_header(8, G.Palette.model(), loop=None)) == 13 + 48
    for bad in (np.zeros((0, 3)), np.zeros((256, 3)), np.zeros((4, 4))):
        with pytest.raises(ValueError):
            G.Palette(bad)
    with pytest.raises(ValueError):
        G.HostEncoder(2, 8, G.Palette.model()).add(np.zeros((1, 8, 8, 3), np.uint8))
    with pytest.raises(ValueError, match="HIP"):
        G.GifEncoder("cpu", 1, 8, G.Palette.model())
    with pytest.raises(ValueError, match="HIP"):
        G.record_episodes(object(), None)


# ------------------------------------------------------------------------------------------ 6. sanitizers
def test_gif_host_code_sanitized(tmp_path):
    """csrc/gif/d2d_gif_core.h (the palette lookup, index + delta, the segmented LZW, the merge, the framing, the
    twin) as a stand-alone program under the address and undefined-behaviour sanitizers: tests/gif_host_main.cpp
    lists the cases.  Nothing is preloaded and nothing sanitized is loaded into Python."""
    from drone2d_amd import _build

    exe = tmp_path / "gif_host"
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-I", os.path.join(_build.PKG_DIR, "csrc"),
                    os.path.join(REPO, "tests", "gif_host_main.cpp"), "-o", str(exe)], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
