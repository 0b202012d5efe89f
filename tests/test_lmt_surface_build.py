"""The local-map tracker surface without a device: tests/cpp/lmt_surface.cpp, written against include/ygz only, compiles and links with
-Wl,--no-undefined; `lmt_surface check` walks the check lists of ygz_hip_map_point_attributes and ygz_hip_stereo_local_map_indexed with a null
context from C++, in the order the header states, and a refused call writes nothing; the class header compiles on its own; the class makes its
three device calls from one place each, shares its gather with LocalMapSelector through a private header, and reads no environment variable."""
import os
import re
import subprocess

from conftest import ROOT

PKG = os.path.join(ROOT, "ygz_slam_amd")
CHECKS = ["mpa_valid_call_wants_a_context", "mpa_nulls_and_counts", "mpa_capacity_before_offsets", "mpa_offsets", "mpa_rows_before_the_rows_are_read",
          "mpa_indices_levels_finiteness", "indexed_valid_call_wants_a_context", "indexed_nulls_and_counts", "indexed_capacity_before_parameters",
          "indexed_parameters", "indexed_map_and_lists", "indexed_finiteness_over_the_whole_map"]


def build_program(out_dir):
    """compile tests/cpp/lmt_surface.cpp into a program in out_dir (also used by tests/test_gpu_lmt_surface.py)"""
    exe = os.path.join(out_dir, "lmt_surface")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-Wall", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "lmt_surface.cpp"), "-o", exe, "-L", PKG, "-lygz_host", "-lygz_hip",
                           "-Wl,--no-undefined", "-Wl,-rpath," + PKG])
    return exe


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
    src.write_text('#include "ygz/Algorithm/LocalMapTracker.h"\n'
                   'int main() { ygz::LocalMapTracker t; ygz::LocalMapTracker::Result r; return t._options._neighbours == 10 && t._options._track._min_edges == 3 && !r.ref && r.status == 1 ? 0 : 1; }\n')
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), str(src)])


def test_public_surface_and_sharing():
    hdr = open(os.path.join(ROOT, "include", "ygz", "Algorithm", "LocalMapTracker.h")).read()
    for decl in [r"int\s+Track\s*\(\s*const\s+std::vector<Frame\s*\*>\s*&\s*frames\s*,\s*std::vector<Result>\s*\*\s*results\s*\)",
                 r"struct\s+Result\s*:\s*StereoLocalMap::Result", r"Frame\s*\*\s*ref\b", r"int\s+voters\b", r"int\s+cut\b", r"struct\s+Stats\b",
                 r"int\s+refused\b", r"int\s+removed\b", r"The host route\W+differs in two ways", r"FAILS the whole\W+call there"]:
        assert re.search(decl, hdr), decl
    assert '#include "ygz/Algorithm/LocalMapTracker.h"' in open(os.path.join(ROOT, "include", "ygz", "Algorithm.h")).read()
    mk = open(os.path.join(PKG, "host", "Makefile")).read()
    assert mk.count("ygz_lmt.cpp") == 2 and "lms_gather.h" in mk
    host = re.sub(r"//[^\n]*", "", open(os.path.join(PKG, "host", "ygz_lmt.cpp")).read())
    lms = re.sub(r"//[^\n]*", "", open(os.path.join(PKG, "host", "ygz_lms.cpp")).read())
    gather = open(os.path.join(PKG, "host", "lms_gather.h")).read()
    # one gather, shared; three device calls, one place each; the selection goes through the selector's one call site
    assert '#include "lms_gather.h"' in host and '#include "lms_gather.h"' in lms and host.count("g.gather(") == 1 and lms.count("g.gather(") == 1
    assert "void gather(" in gather and "unordered_map" in gather
    assert host.count("hip::lms_select(") == 1 and host.count("ygz_hip_map_point_attributes(") == 1 and host.count("ygz_hip_stereo_local_map_indexed(") == 1
    assert host.count("GetCamCenter()") == 1 and "PointAttributes" not in host and "append_point" not in host
    for word in ("Memory::Register", "CreateMapPoint", "StereoTracker", "getenv", "environ"):
        assert word not in host and word not in gather, word
    others = [f for f in os.listdir(os.path.join(PKG, "host")) if f.endswith(".cpp") and f != "ygz_lmt.cpp"]
    for sym in ("ygz_hip_map_point_attributes", "ygz_hip_stereo_local_map_indexed"):
        assert all(sym not in open(os.path.join(PKG, "host", f)).read() for f in others), sym
