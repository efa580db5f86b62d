#!/usr/bin/env python3
"""Writes tests/golden/sflow_*.npz: the inputs of tests/sflow_fixtures.py::CASES and what libviso2's own Matcher (the
reference's src/libviso2, unmodified) computes from them -- its eight feature arrays, getRawMatches() and, for the dense
case (multi_stage = 0, refinement = 0), getMatches().  Data only; the driver is tests/golden/make_sflow_golden.cpp.

Run in the build container:  python tests/golden/make_sflow_golden.py <reference root> [directory for the driver binary]
(without the second argument a temporary directory is made and removed)
Compile line:  g++ -O2 -msse3 -I <ref>/src/libviso2/src make_sflow_golden.cpp matcher.cpp filter.cpp triangle.cpp matrix.cpp"""
import os
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import ref_sflow as rf  # noqa: E402
import sflow_fixtures as sf  # noqa: E402

SETS = ("m1p1", "m2p1", "m1c1", "m2c1", "m1p2", "m2p2", "m1c2", "m2c2")


def build(ref, scratch):
    src = os.path.join(ref, "src", "libviso2", "src")
    exe = os.path.join(scratch, "make_sflow_golden")
    cmd = ["g++", "-O2", "-msse3", "-w", "-I", src, os.path.join(HERE, "make_sflow_golden.cpp")]
    cmd += [os.path.join(src, f) for f in ("matcher.cpp", "filter.cpp", "triangle.cpp", "matrix.cpp")] + ["-o", exe]
    subprocess.check_call(cmd)
    return exe


def run(exe, scratch, name):
    W, H, half, d, motion, method, seed, dense = sf.CASES[name]
    f = sf.frames(W, H, d, motion, seed)
    p = rf.resolve(sf.case_params(name))
    head = np.array([W, H, method, half, 0 if dense else 1, 0 if dense else 1, p["nms_n"], p["nms_tau"], p["match_binsize"],
                     p["match_radius"], p["match_disp_tolerance"], 1], np.int32)
    fin, fout = os.path.join(scratch, "sflow_in.bin"), os.path.join(scratch, "sflow_out.bin")
    with open(fin, "wb") as g:
        g.write(head.tobytes())
        for k in sf.IMAGES:
            g.write(f[k].tobytes())
    subprocess.check_call([exe, fin, fout])
    words = np.fromfile(fout, np.int32)
    out, at = {"img_" + k: f[k] for k in sf.IMAGES}, 0

    def take():
        nonlocal at
        n = int(words[at])
        rec = words[at + 1:at + 1 + 12 * n].reshape(n, 12).copy()
        at += 1 + 12 * n
        return rec
    for s in SETS:
        out[s] = take()
    out["raw_matches"], out["matches"] = take(), take()
    out["cpu_us"] = words[at:at + 2].copy()     # pushBack x 2, matchFeatures: wall time on the machine that wrote the file
    out["method"] = np.int32(method)
    if dense:       # only the dense sets and getMatches() mean anything without the first pass
        for s in SETS[:4]:
            del out[s]
        del out["raw_matches"]
    else:
        del out["matches"]
    path = os.path.join(HERE, "sflow_%s.npz" % name)
    np.savez_compressed(path, **out)
    print(name, {k: (v.shape[0] if v.ndim == 2 and k[0] != "i" else None) for k, v in out.items()}, os.path.getsize(path), "bytes",
          "cpu us", out["cpu_us"].tolist())


def main():
    if len(sys.argv) < 2:
        sys.exit(__doc__)
    ref = sys.argv[1]
    with tempfile.TemporaryDirectory() as tmp:
        scratch = sys.argv[2] if len(sys.argv) > 2 else tmp
        exe = build(ref, scratch)
        for name in sf.CASES:
            run(exe, scratch, name)


if __name__ == "__main__":
    main()
