"""Instruction budget of k_klt3's evaluation loop, checked where it is decided: in the gfx950 assembly of ygz_slam_amd/csrc/klt.hip for
the flags of its Makefile (hipcc cross-compiles without a GPU).  The benchmark step takes the time of its total issue work and LK's
mismatch evaluations are the largest share of it: a change that puts VALU work, crossbar round trips or address
arithmetic back into the loop costs time and shows up in no parity test.

The loop is the one at depth 2 of the kernel (levels, then iterations): every basic block whose loop annotation says Depth=2 -- for the
loop header that is the second line of its annotation ("Parent Loop ... Depth=1", then "This Inner Loop Header: Depth=2")."""
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

# per wavefront (three points) and evaluation, every block of the loop counted, its header included.  Before this budget the loop issued
# 226 VALU and 12 ds_bpermute (hipcc of ROCm 7.2); it now issues 182 and 8: three instructions under the VALU budget.  The +16 / +8 / +4
# steps and the broadcast of the two segment sums stay on the crossbar.
MAX_VALU = 185
MAX_BPERMUTE = 8
ROW_GATHERS = 4


def _loop_mnemonics():
    r = subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-ffp-contract=off", "-fno-fast-math",
                        "-I" + os.path.join(ROOT, "include"), "--cuda-device-only", "-S", "klt.hip", "-o", "-"],
                       cwd=CSRC, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = r.stdout.splitlines()
    i0 = next(i for i, ln in enumerate(lines) if ln.startswith(KERNEL + ":"))
    i1 = next(i for i in range(i0, len(lines)) if lines[i].strip().startswith(".Lfunc_end"))
    depth, at_label, out = 0, False, collections.Counter()
    for ln in lines[i0 + 1:i1]:
        if re.match(r"^(\.LBB\d+_\d+:|; %bb\.\d+:)", ln):             # a basic block; its loop depth is in the annotation
            m = re.search(r"Depth=(\d+)", ln)
            depth, at_label = (int(m.group(1)) if m else 0), True
            continue
        s = ln.strip()
        if at_label and s.startswith(";"):
            # a loop header says "Parent Loop ... Depth=1" on its label line and its own depth on the next one
            # ("; =>  This Inner Loop Header: Depth=2"): the header block runs on every iteration and is part of the loop
            m = re.search(r"Loop Header: Depth=(\d+)", s)
            if m:
                depth = int(m.group(1))
            continue
        at_label = False
        if depth == 2 and s and s[0] not in ";." and not s.endswith(":"):
            out[s.split()[0]] += 1
    return out


@pytest.mark.skipif(shutil.which(HIPCC) is None and not os.path.exists(HIPCC), reason="hipcc not available")
def test_klt3_evaluation_loop_budget():
    c = _loop_mnemonics()
    valu = sum(v for k, v in c.items() if k.startswith("v_"))
    gathers = sum(v for k, v in c.items() if k.startswith(("global_load", "buffer_load", "flat_load")))
    report = "VALU %d (budget %d), ds_bpermute %d (budget %d), vector loads %s" % (
        valu, MAX_VALU, c["ds_bpermute_b32"], MAX_BPERMUTE, {k: v for k, v in c.items() if k.startswith(("global_", "buffer_", "flat_"))})
    assert valu <= MAX_VALU, report
    assert c["ds_bpermute_b32"] <= MAX_BPERMUTE, report
    # exactly the four window rows, as three aligned dwords each, and no other vector-memory or LDS-array access
    assert c["global_load_dwordx3"] == ROW_GATHERS and gathers == ROW_GATHERS, report
    assert not [k for k in c if k.startswith(("ds_read", "ds_write", "global_store", "scratch_", "buffer_store"))], report
    # FP64 is left only in the squared-step test (one fma)
    assert sum(v for k, v in c.items() if k.startswith("v_cmp") and "f64" in k) <= 1, report
