"""k_klt3 keeps the window of the current image between mismatch evaluations: the row gathers, their realignment and the unpacking into
pixel pairs run only when a lane that iterates is on new pixels (ygz_slam_amd/csrc/klt.hip).  Checked in the gfx950 assembly, with the
pipeline of tests/test_klt_isa_budget.py: in the depth-2 loop of the kernel, the basic blocks that hold the four gathers hold every
v_alignbyte and the v_perm_b32 of all kept rows, and a block without a vector load -- what an evaluation on kept pixels runs -- holds
none of the realignment."""
import collections
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "ygz_slam_amd", "csrc")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
KERNEL = "_Z6k_klt37KltArgs"
ROWS_KEPT = 4                  # window rows kept as unpacked pairs, 7 v_perm_b32 each
LOADS = ("global_load", "buffer_load", "flat_load")


def _loop_blocks():
    """[Counter of mnemonics] per basic block of the loop at depth 2, its header included"""
    r = subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-ffp-contract=off", "-fno-fast-math",
                        "-I" + os.path.join(ROOT, "include"), "--cuda-device-only", "-S", "klt.hip", "-o", "-"],
                       cwd=CSRC, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = r.stdout.splitlines()
    i0 = next(i for i, ln in enumerate(lines) if ln.startswith(KERNEL + ":"))
    i1 = next(i for i in range(i0, len(lines)) if lines[i].strip().startswith(".Lfunc_end"))
    blocks, depth, at_label = [], 0, False
    for ln in lines[i0 + 1:i1]:
        if re.match(r"^(\.LBB\d+_\d+:|; %bb\.\d+:)", ln):
            m = re.search(r"Depth=(\d+)", ln)
            depth, at_label = (int(m.group(1)) if m else 0), True
            blocks.append([depth, collections.Counter()])
            continue
        s = ln.strip()
        if at_label and s.startswith(";"):
            m = re.search(r"Loop Header: Depth=(\d+)", s)          # a loop header carries its own depth on the second line of its annotation
            if m:
                blocks[-1][0] = int(m.group(1))
            continue
        at_label = False
        if blocks and s and s[0] not in ";." and not s.endswith(":"):
            blocks[-1][1][s.split()[0]] += 1
    return [c for d, c in blocks if d == 2]


def _valu(c):
    return sum(v for k, v in c.items() if k.startswith("v_"))


@pytest.mark.skipif(shutil.which(HIPCC) is None and not os.path.exists(HIPCC), reason="hipcc not available")
def test_klt3_reload_is_confined_to_the_gather_blocks():
    blocks = _loop_blocks()
    assert blocks, "no loop at depth 2 in k_klt3"
    with_load = [c for c in blocks if any(k.startswith(LOADS) for k in c)]
    without = [c for c in blocks if not any(k.startswith(LOADS) for k in c)]
    gathers = sum(v for c in with_load for k, v in c.items() if k.startswith(LOADS))
    align_all = sum(c["v_alignbyte_b32"] for c in blocks)
    align_in = sum(c["v_alignbyte_b32"] for c in with_load)
    perm_in = sum(c["v_perm_b32"] for c in with_load)
    print("k_klt3 evaluation loop: %d VALU in the blocks without a vector load (the evaluation on kept pixels), %d in the blocks with the gathers"
          % (sum(_valu(c) for c in without), sum(_valu(c) for c in with_load)))
    assert gathers == 4 and sum(c["global_load_dwordx3"] for c in with_load) == 4, [dict(c) for c in with_load]
    assert align_all > 0 and align_in == align_all, (align_in, align_all)
    assert perm_in >= 7 * ROWS_KEPT, perm_in
    assert not any(c["v_alignbyte_b32"] for c in without)
