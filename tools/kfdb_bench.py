#!/usr/bin/env python3
"""Call time of ygz_hip_kfdb_query (the keyframe database, csrc/kfdb.hip) beside the way it replaces: common words counted and
DBoW3::Vocabulary::score called per keyframe over std::map BoW vectors on one host core, timed inside the C++ program of the tests
(tests/cpp/kfdb_surface.cpp: kfdb_host_loop_ms).  Vectors: tests/kfdb_ref.py's synthetic ones, 1000 words each out of a 10^6-word vocabulary
with a Zipf-like word frequency, L1-normalised (two vectors share about 90 words).  Databases of 4 .. 4096 keyframes (64, 512 and 4096 are the sizes that matter; the small ones
locate the crossover); 1 and 64 queries per call.  Per row: the wall time of the C ABI call (one upload, the launch, one copy back, one wait;
the arrays are marshalled outside the clock), 5 warm-up calls then 30 timed, median / p10 / p90; the device time of the same call through
ygz_hip_timer_begin / _end, median of 20; the host loop's median over 21 passes for one query (the 64-query figure is 64 times that: the loop
has nothing to share between queries); the cost of one add (all rows added back to back, then one wait, divided by the rows); whether the
device's numbers equal the host loop's bit for bit.  Usage (on the GPU box): tools/kfdb_bench.py [out.json] [--lib libygz_hip.so]
[--program libkfdb_surface.so]; the default output is profiles/kfdb_bench.json."""
import ctypes as C
import datetime
import json
import os
import platform
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import kfdb_ref as kr                         # noqa: E402  (test infrastructure: the vectors and the one-core restatement)
from ygz_slam_amd import _lib                 # noqa: E402

SIZES = (4, 8, 16, 32, 64, 512, 4096)
QUERIES = (1, 64)
WORDS, SPACE = 1000, 10 ** 6


def stats(ts):
    ts = np.asarray(ts) * 1e3
    return dict(median_ms=float(np.median(ts)), p10_ms=float(np.percentile(ts, 10)), p90_ms=float(np.percentile(ts, 90)), calls=len(ts))


def device_name():
    try:
        import torch
        return torch.cuda.get_device_name(0)
    except Exception:                         # noqa: BLE001
        return "unknown"


def option(name):
    if name in sys.argv:
        i = sys.argv.index(name)
        v = sys.argv[i + 1]
        del sys.argv[i:i + 2]
        return v
    return None


def main():
    lib_path, program_path = option("--lib"), option("--program")
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "kfdb_bench.json")
    if lib_path:
        _lib.LIB_PATH = os.path.abspath(lib_path)
    if not program_path:
        from test_kfdb_surface_build import build_program
        program_path = build_program(tempfile.mkdtemp(prefix="kfdb_bench_"))
    program = C.CDLL(program_path)
    program.kfdb_host_loop_ms.restype = C.c_double
    program.kfdb_host_loop_ms.argtypes = [C.c_int] + [C.c_void_p] * 5 + [C.c_int, C.c_int, C.c_void_p, C.c_void_p]
    vp = lambda a: a.ctypes.data_as(C.c_void_p)
    ctx = _lib.HipContext(width=640, height=480, levels=3, max_frames=2)
    lib = ctx.lib
    rng = np.random.default_rng(4096)
    vectors = kr.synthetic(rng, max(SIZES) + max(QUERIES), WORDS, SPACE)                 # one vocabulary: the frequent words are the same for all
    vectors, queries = vectors[:max(SIZES)], vectors[max(SIZES):]
    rows = []
    for n in SIZES:
        db = _lib.KeyframeDatabase(ctx)
        ctx.synchronize()
        t0 = time.perf_counter()
        for v in vectors[:n]:
            db.add(*v)
        ctx.synchronize()
        add_us = (time.perf_counter() - t0) / n * 1e6
        r_off, r_word, r_weight = kr.pack(vectors[:n])
        host_common, host_score = np.zeros(n, np.int32), np.zeros(n)
        host = []
        for q in range(3):
            qw, qv = queries[q]
            host.append(program.kfdb_host_loop_ms(n, vp(r_off), vp(r_word), vp(r_weight), vp(qw), vp(qv), len(qw), 7, vp(host_common), vp(host_score)))
        qw, qv = queries[0]
        host_ms = float(np.median(host))
        program.kfdb_host_loop_ms(n, vp(r_off), vp(r_word), vp(r_weight), vp(qw), vp(qv), len(qw), 1, vp(host_common), vp(host_score))
        for nq in QUERIES:
            off, word, weight = _lib.kfdb_pack(queries[:nq])
            common, score = np.zeros((nq, n), np.int32), np.zeros((nq, n))
            ip, dp = C.POINTER(C.c_int32), C.POINTER(C.c_double)
            args = (db._db, nq, off.ctypes.data_as(ip), word.ctypes.data_as(ip), weight.ctypes.data_as(dp), common.ctypes.data_as(ip),
                    score.ctypes.data_as(dp))
            wall = []
            for k in range(35):
                t0 = time.perf_counter()
                rc = lib.ygz_hip_kfdb_query(*args)
                t1 = time.perf_counter()
                assert rc == 0, rc
                if k >= 5:
                    wall.append(t1 - t0)
            dev = []
            for k in range(20):
                ctx.timer_begin()
                rc = lib.ygz_hip_kfdb_query(*args)
                dev.append(ctx.timer_end())
                assert rc == 0, rc
            same = np.array_equal(common[0], host_common) and np.array_equal(score[0].view(np.uint64), host_score.view(np.uint64))
            row = dict(keyframes=n, queries=nq, words_per_vector=WORDS, common_mean=float(common.mean()), device=stats(wall),
                       device_timer_ms=float(np.median(dev)), host_loop_ms=host_ms * nq, host_loop_ms_per_query=host_ms, add_us_per_row=add_us,
                       bit_identical=bool(same))
            row["host_over_device"] = row["host_loop_ms"] / row["device"]["median_ms"]
            rows.append(row)
            print(json.dumps(row), flush=True)
        db.close()
    ctx.close()
    cross = {}
    for nq in QUERIES:
        faster = [r["keyframes"] for r in rows if r["queries"] == nq and r["host_over_device"] > 1.0]
        cross[str(nq)] = min(faster) if faster else None
    doc = dict(tool="tools/kfdb_bench.py", date=datetime.date.today().isoformat(), device=device_name(), host=platform.processor() or platform.machine(),
               library=os.path.relpath(_lib.LIB_PATH, ROOT), vectors=dict(words=WORDS, vocabulary=SPACE, frequency="rank^-0.9"), warmup=5, timed=30,
               smallest_database_where_the_device_is_faster=cross, rows=rows)
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
