#!/usr/bin/env python3
"""Times Engine.mars_heightfield on the GPU and its numpy restatement (tests/mars_ref.py) on the CPU, and splits the wall time of
assets.build_mars_scene by stage (EXPERIMENTS.md §28).

    python tools/mars_timing.py [--width 60] [--scales 0.1 0.025] [--reps 9] [--scene] [--json out.json]

Per scale: the planner (host Python), the descriptor, the per-tile list build on its own (rover_mars_tiles: the same host code the call
runs), then one whole rover_mars_heightfield call between two device events — the call is synchronous, so that is its wall time: the
list build, the uploads, the launch and the final synchronisation —, median (min .. max) over --reps calls after two warm-up calls; the
result is compared bit for bit with mars_ref's sequential loop, whose time on this machine's CPU is printed next to it (exit status 1 on
a difference).  --scene: assets.build_mars_scene's stages for the default 60 m yard, one run each.  Needs a GPU; there is no fallback."""
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

from isaac_rover_amd import _lib, assets, terrain_gen  # noqa: E402


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    out = fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b), out


def wall(fn, reps=1):
    """-> (median seconds, result of the last call); the device is idle before and after each call"""
    ts = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        ts.append(time.perf_counter() - t)
    return statistics.median(ts), out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--width", type=float, default=60.0)
    ap.add_argument("--scales", type=float, nargs="+", default=[0.1, 0.025])
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--scene", action="store_true", help="also split one assets.build_mars_scene of the 60 m yard by stage")
    ap.add_argument("--json", default="")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("mars_timing: needs a GPU")
    import mars_ref
    eng = _lib.Engine(1, device=0)
    result = {"version": _lib.version(), "reps": args.reps, "width": args.width, "scales": {}}
    bad = 0
    for hs in args.scales:
        plan_s, plan = wall(lambda: terrain_gen.plan_mars_terrain(args.width, hs))
        desc_s, (desc, keep) = wall(lambda: _lib.mars_plan_desc(plan))
        tiles_s, (start, items) = wall(lambda: _lib.mars_tiles(desc), 5)
        for _ in range(2):
            eng.mars_heightfield(desc)
        ms = []
        for _ in range(args.reps):
            m, (hf, mask) = timed(lambda: eng.mars_heightfield(desc))
            ms.append(m)
        t = time.perf_counter()
        want, want_mask = mars_ref.apply_plan(plan)
        ref_s = time.perf_counter() - t
        same = bool(np.array_equal(mars_ref.bits(hf.cpu().numpy()), mars_ref.bits(want))) and bool(np.array_equal(mask.cpu().numpy(), want_mask))
        bad += not same
        rec = {"nodes": plan.side, "hills": len(plan.hill_amp), "stamps_kept": int(plan.stamp_kept.sum()), "stamps": len(plan.stamp_kept),
               "tile_items": len(items), "longest_tile_list": int(np.diff(start).max()), "plan_s": plan_s, "desc_s": desc_s, "tiles_s": tiles_s,
               "call_ms": (statistics.median(ms), min(ms), max(ms)), "ref_s": ref_s, "check": "equal" if same else "DIFFERENT"}
        result["scales"][str(hs)] = rec
        print(f"--- {args.width} m at {hs} m: {plan.side}^2 nodes ({8 * plan.side ** 2 / 1e6:.1f} MB of float64), {rec['hills']} hills, "
              f"{rec['stamps_kept']} of {rec['stamps']} stamps kept, {rec['tile_items']} tile items, longest list {rec['longest_tile_list']}")
        print(f"planner {1e3 * plan_s:.2f} ms, descriptor {1e3 * desc_s:.3f} ms, tile lists alone (host) {1e3 * tiles_s:.3f} ms")
        print(f"rover_mars_heightfield {rec['call_ms'][0]:.3f} ms ({rec['call_ms'][1]:.3f} .. {rec['call_ms'][2]:.3f}) per call, {args.reps} calls")
        print(f"mars_ref sequential loop on the CPU: {1e3 * ref_s:.1f} ms; check: {rec['check']}")
    if args.scene:
        stages = {}
        stages["plan"], plan = wall(lambda: terrain_gen.plan_mars_terrain(60.0, 0.1))
        stages["mars_heightfield"], (hf, mask) = wall(lambda: eng.mars_heightfield(plan))
        stages["meshes"], (verts, tris, rock_tris) = wall(lambda: assets.mars_meshes(eng, plan, 200))
        stages["meshes"] -= stages["mars_heightfield"]                 # mars_meshes makes the call again
        stages["knn_terrain"], terrain = wall(lambda: assets.build_knn_map(eng, verts, tris))
        stages["knn_rocks"], rocks = wall(lambda: assets.build_knn_map(eng, verts, rock_tris))
        stages["heightfield_and_stones"], _ = wall(lambda: assets._scene_on_maps(eng, terrain, rocks, (verts, rock_tris), 600, 0.1, 0.025, (0.0, 0.0, 0.0), None))
        stages["whole_build_mars_scene"], (scene, _) = wall(lambda: assets.build_mars_scene(eng))
        result["scene"] = dict(stages, triangles=len(tris), rock_triangles=len(rock_tris), stones=len(scene.stone_info_raw))
        print(f"--- build_mars_scene, 60 m yard: {len(tris)} triangles, {len(rock_tris)} rock triangles, {len(scene.stone_info_raw)} stones")
        for k, v in stages.items():
            print(f"{k:24s} {v:8.3f} s")
    eng.close()
    if args.json:
        with open(args.json, "w") as fh:
            json.dump(result, fh, indent=1)
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
