"""The resident-map surface without a device: the new symbols are bound by the loader, exported and declared, and the structs have the sizes
the header states; tests/cpp/rmap_surface.cpp, written against include/ygz only, compiles and links with -Wl,--no-undefined, and
`rmap_surface check` walks the check lists of ygz_hip_map_upload, ygz_hip_map_update and ygz_hip_stereo_local_map_resident with a null context
from C++, in the order the header states, and a refused call writes nothing; the class header compiles on its own; the class shares its
gathers and its write-back with LocalMapTracker instead of copying them, and makes its device calls from one place each."""
import ctypes
import os
import re
import subprocess

from conftest import ROOT

PKG = os.path.join(ROOT, "ygz_slam_amd")
CHECKS = ["object_calls_want_a_context", "upload_valid_call_wants_a_context", "upload_selection_nulls_and_counts",
          "upload_selection_capacity_before_offsets_and_attributes", "upload_selection_arrays_before_attributes", "upload_attribute_side",
          "upload_descriptor_last", "update_wants_a_context_and_a_map", "resident_valid_call_wants_a_context", "resident_nulls_and_counts",
          "resident_capacity_before_parameters", "resident_parameters_and_pairs_before_offsets", "resident_offsets_then_the_context"]
NEW_SOURCES = [os.path.join(PKG, "csrc", f) for f in ("rmap.hip", "rmap_host.h", "lms_dev.h", "mpa_dev.h")] + \
              [os.path.join(PKG, "host", f) for f in ("ygz_rmap.cpp", "lmt_share.h")] + \
              [os.path.join(ROOT, "tests", "rmap_ref.py"), os.path.join(ROOT, "tools", "rmap_bench.py")]


def build_program(out_dir):
    """compile tests/cpp/rmap_surface.cpp into a program in out_dir (also used by tests/test_gpu_rmap_surface.py)"""
    exe = os.path.join(out_dir, "rmap_surface")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-Wall", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "rmap_surface.cpp"), "-o", exe, "-L", PKG, "-lygz_host", "-lygz_hip",
                           "-Wl,--no-undefined", "-Wl,-rpath," + PKG])
    return exe


def test_symbols_struct_sizes_and_ids(hip_lib):
    lib = hip_lib.load()
    hdr = open(os.path.join(ROOT, "include", "ygz_hip.h")).read()
    assert hip_lib.RMAP_SYMBOLS == ["ygz_hip_map_create", "ygz_hip_map_destroy", "ygz_hip_map_info", "ygz_hip_map_upload", "ygz_hip_map_update",
                                    "ygz_hip_map_download", "ygz_hip_stereo_local_map_resident"]
    assert re.search(r"Still 6: the resident map added", hdr)
    assert hip_lib.ABI_VERSION == 6 == lib.ygz_hip_abi_version() and re.search(r"#define\s+YGZ_HIP_ABI_VERSION\s+6\b", hdr)
    for s in hip_lib.RMAP_SYMBOLS:
        assert s in hip_lib.ABI_SYMBOLS and hasattr(lib, s), s
        assert re.search(r"\bint\s+%s\s*\(" % s, hdr), s
    assert ctypes.sizeof(hip_lib.MapArrays) == 120 and ctypes.sizeof(hip_lib.MapInfo) == 40 and "sizeof: ygz_map_arrays 120, ygz_map_info 40" in hdr
    # the C compiler agrees
    fields = re.search(r"typedef struct \{([^}]*)\} ygz_map_arrays;", hdr).group(1)
    assert len(re.findall(r"\*\s*\w+", fields)) == 13 and len(re.findall(r"\bn_\w+", fields.split(";")[0])) == 4
    assert [n for n, _ in hip_lib.MapArrays._fields_] == re.findall(r"\b(?:n_\w+|kf_bad|cov|offsets|kf|feat|pt_bad|centre|a_offsets|a_kf|a_level|pw|pt_desc|pt_has_desc)\b", fields)
    internal = open(os.path.join(PKG, "csrc", "ygz_internal.h")).read()
    assert re.search(r"#define\s+YGZ_N_SCRATCH\s+48\b", internal) and "std::vector<ygz_hip_map *> maps;" in internal
    for path in NEW_SOURCES:
        code = re.sub(r"//[^\n]*", "", open(path).read())
        assert "getenv" not in code and "environ" not in code, path
    mk = open(os.path.join(PKG, "csrc", "Makefile")).read()
    # every object depends on every header of csrc/, these three among them
    assert "$(wildcard *.h)" in re.search(r"build/%\.o:[^\n]*", mk).group(0) and "$(wildcard *.hip)" in mk
    assert all(os.path.exists(os.path.join(PKG, "csrc", h)) for h in ("rmap_host.h", "lms_dev.h", "mpa_dev.h"))


def test_struct_size_from_the_c_compiler(tmp_path):
    src = tmp_path / "size.c"
    src.write_text('#include "ygz_hip.h"\n#include <stddef.h>\n'
                   '_Static_assert(sizeof(ygz_map_arrays) == 120 && sizeof(ygz_map_info) == 40, "sizes");\n'
                   '_Static_assert(offsetof(ygz_map_arrays, kf_bad) == 16 && offsetof(ygz_map_arrays, pt_has_desc) == 112, "offsets");\n'
                   '_Static_assert(offsetof(ygz_map_info, resident_bytes) == 32, "info");\nint main(void) { return 0; }\n')
    subprocess.check_call(["gcc", "-std=c11", "-Wall", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), str(src)])


def test_program_links_and_walks_the_check_lists(tmp_path):
    assert os.path.exists(os.path.join(PKG, "libygz_host.so")), "libygz_host.so is not built (run __graft_entry__.build())"
    exe = build_program(str(tmp_path))
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60)          # no arguments: the usage line, no device touched
    assert r.returncode == 2 and "usage" in r.stderr
    r = subprocess.run([exe, "check"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, (r.returncode, r.stdout, r.stderr[-2000:])
    assert r.stdout.split("\n")[:-1] == [c + " ok" for c in CHECKS], r.stdout


def test_class_header_compiles_against_include_ygz(tmp_path):
    src = tmp_path / "only.cpp"
    src.write_text('#include "ygz/Algorithm/ResidentMap.h"\n'
                   'int main() { ygz::ResidentMap::Options o; ygz::ResidentMap::Result r; ygz::ResidentMap::Stats s; '
                   'return o._neighbours == 10 && o._track._min_edges == 3 && !r.ref && s.uploads == 0 ? 0 : 1; }\n')
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), str(src)])


def test_public_surface_and_sharing():
    hdr = open(os.path.join(ROOT, "include", "ygz", "Algorithm", "ResidentMap.h")).read()
    for decl in [r"bool\s+Upload\s*\(\s*const\s+std::vector<Frame\s*\*>\s*&\s*keyframes\s*\)",
                 r"int\s+Update\s*\(\s*const\s+std::vector<MapPoint\s*\*>\s*&\s*points\s*,\s*const\s+std::vector<Frame\s*\*>\s*&\s*keyframes\s*\)",
                 r"int\s+Track\s*\(\s*const\s+std::vector<Frame\s*\*>\s*&\s*frames\s*,\s*std::vector<Result>\s*\*\s*results\s*\)",
                 r"typedef\s+LocalMapTracker::Result\s+Result", r"When the two routes agree", r"a superset changes no outcome",
                 r"What makes the resident map stale", r"int\s+skipped\b", r"int\s+unknown\b"]:
        assert re.search(decl, hdr), decl
    assert '#include "ygz/Algorithm/ResidentMap.h"' in open(os.path.join(ROOT, "include", "ygz", "Algorithm.h")).read()
    mk = open(os.path.join(PKG, "host", "Makefile")).read()
    assert mk.count("ygz_rmap.cpp") == 2 and "lmt_share.h" in mk and "lms_gather.h" in mk
    host = re.sub(r"//[^\n]*", "", open(os.path.join(PKG, "host", "ygz_rmap.cpp")).read())
    lmt = re.sub(r"//[^\n]*", "", open(os.path.join(PKG, "host", "ygz_lmt.cpp")).read())
    share = open(os.path.join(PKG, "host", "lmt_share.h")).read()
    gather = open(os.path.join(PKG, "host", "lms_gather.h")).read()
    # the gathers and the write-back exist once and both classes go through them
    assert '#include "lms_gather.h"' in host and '#include "lmt_share.h"' in host and '#include "lmt_share.h"' in lmt
    assert host.count("g.gather_map(") == 1 and "void gather_map(" in gather and gather.count("void build(") == 1 and gather.count("build(frames, neighbours, kf_at);") == 1
    assert host.count("rows.collect(") == 1 and lmt.count("rows.collect(") == 1 and lmt.count("void LmtRows::collect(") == 1 and "void collect(" in share
    assert host.count("hip::lmt_apply(") == 1 and lmt.count("hip::lmt_apply(") == 1 and lmt.count("int lmt_apply(") == 1 and "int lmt_apply(" in share
    assert "_cnt_visible" not in host and "_track_in_view" not in host and "apply_verdict" not in host and "_distinctive_desc" not in host
    # one place per device call
    for sym in ("ygz_hip_map_create(", "ygz_hip_map_destroy(", "ygz_hip_map_upload(", "ygz_hip_map_update(", "ygz_hip_stereo_local_map_resident("):
        assert host.count(sym) == 1, sym
    others = [f for f in os.listdir(os.path.join(PKG, "host")) if f.endswith(".cpp") and f != "ygz_rmap.cpp"]
    for sym in ("ygz_hip_map_upload", "ygz_hip_map_update", "ygz_hip_stereo_local_map_resident"):
        assert all(sym not in open(os.path.join(PKG, "host", f)).read() for f in others), sym
    for word in ("Memory::Register", "CreateMapPoint", "StereoTracker", "getenv", "environ"):
        assert word not in host and word not in share, word
