#!/bin/bash
# Device assembly of the product library + per-kernel resource summary (CPU container).
# Usage: bash tools/isa.sh [out.s] [extra hipcc flags...]
# The last column hashes each kernel's body with what moves between two compiles of unchanged device
# code taken out (the function index in .LBB<i>_ labels and the file-wide count in .Lpost_getpc<k>
# labels, which follow instantiation order, and the random __hip_cuid_ symbol): a host-only change
# leaves every row as it was; rows are sorted by name.
# ISA_ONLY=1: summarise an existing out.s without compiling.
set -e
R=$(cd "$(dirname "$0")/.." && pwd)
OUT=${1:-/tmp/d2d_isa.s}; shift || true
[ -n "$ISA_ONLY" ] || /opt/rocm/bin/hipcc --offload-arch=gfx950 -O3 -std=c++17 -ffp-contract=off -fno-fast-math -Wall -Werror \
  -Wno-unused-command-line-argument -I"$R/include" --cuda-device-only -S -o "$OUT" "$@" \
  "$R/drone-2d-custom-gym-env-for-reinforcement-learning_amd/csrc/d2d_hip.hip"
python3 - "$OUT" <<'PY'
import hashlib, re, sys
t = open(sys.argv[1]).read()
for name in sorted(re.findall(r"^(_ZN4d2dk\w+):", t, re.M)):
    blk = t[t.index("\n" + name + ":") + 1:]
    g = lambda k: (re.search(r"; " + k + r":\s*(\d+)", blk) or [None, "?"])[1]
    body = blk[:re.search(r"^\.Lfunc_end\d+:", blk, re.M).start()]
    body = re.sub(r"BB\d+_", "BB_",re.sub(r"__hip_cuid_\w+", "__hip_cuid", body))
    body = re.sub(r"\.Lpost_getpc\d+", ".Lpost_getpc", body)  # (long-branch labels: numbered through the file)
    body = re.sub(r"[ \t]+", " ", body)  # (comments are aligned after the label, whose width moves)
    h = hashlib.sha256(body.encode()).hexdigest()[:12]
    print(f"{name:60s} vgpr {g('NumVgprs')} agpr {g('NumAgprs')} spill {g('ScratchSize')} lds {g('LDSByteSize') } occ {g('Occupancy')} {h}")
PY
