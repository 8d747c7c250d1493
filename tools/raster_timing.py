#!/usr/bin/env python3
"""Times rover_build_heightfield on the GPU and its numpy restatement (tests/raster_ref.py) on the CPU (EXPERIMENTS.md §24).

    python tools/raster_timing.py [--inputs grid irregular] [--reps 9] [--check] [--json out.json]

  grid        synth.grid_mesh(601): 720 000 triangles of a 0.1 m grid -> 2 400 x 2 400 nodes at 0.025 m (every box 5 x 5 nodes: small route)
  irregular   synth.irregular_mesh(IrregularSpec()): the default 10 m x 10 m decimated-style mesh -> 400 x 400 nodes (both routes)
A figure is one whole call between two device events — the call is synchronous, so that is its wall time: uploads, the memset, the
launches, the read of the list's length, the decode and the final synchronisation —, median (min .. max) over --reps calls after two
warm-up calls, once with the mesh in host memory (what assets.build_scene_from_meshes passes) and once with it on the device.
--check runs the restatement once per input, reports its time and compares the full-size result bit for bit (exit status 1 on a
difference); it also counts the covered (node, triangle) pairs, which is the number of atomics of a call.  The bytes of a call are
computed from the sizes: node array cleared (4 N), decoded in place (8 N), one 4-byte atomic per covered pair, 12 V + 12 T read and
16 V written by the snap pass, 12 T + 48 T read by the triangle pass.  Needs a GPU; there is no fallback."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from isaac_rover_amd import _lib, synth  # noqa: E402


def make_input(name):
    """-> (vertices, triangles, n0, n1)"""
    if name == "grid":
        verts, tris, _ = synth.grid_mesh(601)
        return verts, tris, 2400, 2400
    spec = synth.IrregularSpec()
    verts, tris, _, _ = synth.irregular_mesh(spec)
    return verts, tris, int(round(spec.extent_x / 0.025)), int(round(spec.extent_y / 0.025))


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    out = fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b), out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--inputs", nargs="+", default=["grid", "irregular"], choices=["grid", "irregular"])
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--check", action="store_true", help="run tests/raster_ref.py on the full-size input and compare bit for bit")
    ap.add_argument("--json", default="")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("raster_timing: needs a GPU")
    eng = _lib.Engine(1, device=0)
    result = {"version": _lib.version(), "reps": args.reps, "limits": _lib.heightfield_limits(), "inputs": {}}
    bad = 0
    for name in args.inputs:
        verts, tris, n0, n1 = make_input(name)
        dv, dt = torch.from_numpy(verts).to(eng.device), torch.from_numpy(tris).to(eng.device)
        rec = {"vertices": len(verts), "triangles": len(tris), "nodes": [n0, n1]}
        for label, v, t in (("host_inputs", verts, tris), ("device_inputs", dv, dt)):
            for _ in range(2):
                out = eng.build_heightfield(v, t, n0, n1, 0.025, (0.0, 0.0), -1.0)
            ms = []
            for _ in range(args.reps):
                m, out = timed(lambda: eng.build_heightfield(v, t, n0, n1, 0.025, (0.0, 0.0), -1.0))
                ms.append(m)
            rec[label + "_ms"] = (statistics.median(ms), min(ms), max(ms))
        hm, uncovered, skipped = out
        rec["uncovered"], rec["skipped"] = uncovered, skipped
        n, V, T = n0 * n1, len(verts), len(tris)
        rec["bytes_fixed"] = 12 * n + 28 * V + 72 * T
        print(f"--- {name}: {T} triangles, {V} vertices -> {n0} x {n1} nodes ({4 * n / 1e6:.1f} MB), {uncovered} uncovered, {skipped} skipped")
        for label in ("host_inputs", "device_inputs"):
            med, lo, hi = rec[label + "_ms"]
            print(f"{label:14s} {med:9.3f} ms ({lo:.3f} .. {hi:.3f}) per call, {args.reps} calls")
        print(f"bytes without the atomics: {rec['bytes_fixed'] / 1e6:.1f} MB = {rec['bytes_fixed'] / (4 * n):.2f} x the node array")
        if args.check:
            import raster_ref
            t0 = time.perf_counter()
            want, w_unc, w_skip, count, _ = raster_ref.build_heightfield(verts, tris, n0, n1, 0.025, (0.0, 0.0), -1.0, return_count=True)
            rec["ref_s"] = time.perf_counter() - t0
            rec["covered_pairs"] = int(count.sum())
            got = hm.cpu().numpy()
            differ = int((got.view(np.uint32) != want.view(np.uint32)).sum())
            same = differ == 0 and (uncovered, skipped) == (w_unc, w_skip)
            rec["check"] = "equal" if same else f"{differ} nodes differ, stats {(uncovered, skipped)} vs {(w_unc, w_skip)}"
            bad += not same
            total = rec["bytes_fixed"] + 4 * rec["covered_pairs"]
            print(f"raster_ref on the CPU: {rec['ref_s']:.1f} s; {rec['covered_pairs']} covered (node, triangle) pairs = atomics; "
                  f"bytes with them {total / 1e6:.1f} MB = {total / (4 * n):.2f} x the node array; check: {rec['check']}")
        result["inputs"][name] = rec
    eng.close()
    if args.json:
        with open(args.json, "w") as fh:
            json.dump(result, fh, indent=1)
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
