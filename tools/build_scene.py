#!/usr/bin/env python3
"""CLI of assets.generate_scene_files — everything a Scene needs from the two meshes of a terrain directory: reads map.ply (terrain with
rocks) and big_stones.ply (rocks only) and writes knn_terrain/, knn_rocks/, heightmap_tensor.pt and stone_info.npy next to them, in the
layout assets.load_reference_assets reads.

    python tools/build_scene.py /path/to/omniisaacgymenvs/tasks/utils/terrain [--cells 600 --res 0.1 --k 200 --hscale 0.025]

``--mars SEED [--width 60]`` first GENERATES the two meshes with the reference's Mars terrain generator (terrain_gen.plan_mars_terrain at
``--res`` metres per node, Engine.mars_heightfield) and writes them as map.ply and big_stones.ply into the directory.
"""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main(argv=None, make_engine=None):
    """``make_engine``: a stand-in for ``lambda: _lib.Engine(1, device=0)`` (the tests run the file layout without a GPU)."""
    from isaac_rover_amd import assets
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("terrain_dir")
    ap.add_argument("--cells", type=int, default=600, help="map cells per side")
    ap.add_argument("--res", type=float, default=0.1, help="metres per map cell")
    ap.add_argument("--k", type=int, default=200, help="triangles per map cell")
    ap.add_argument("--hscale", type=float, default=0.025, help="metres per heightfield node")
    ap.add_argument("--ranking", default="exact_f32", choices=["exact_f32", "reference_fp16"])
    ap.add_argument("--mars", type=int, default=None, metavar="SEED", help="generate map.ply and big_stones.ply from this seed first")
    ap.add_argument("--width", type=float, default=60.0, help="with --mars: side of the generated yard in metres")
    a = ap.parse_args(argv)
    if make_engine is None:
        from isaac_rover_amd import _lib
        make_engine = lambda: _lib.Engine(1, device=0)  # noqa: E731
    eng = make_engine()
    t = time.perf_counter()
    if a.mars is not None:
        from isaac_rover_amd import terrain_gen
        plan = terrain_gen.plan_mars_terrain(a.width, a.res, seed=a.mars)
        verts, tris, rock_tris = assets.mars_meshes(eng, plan, a.k)
        os.makedirs(a.terrain_dir, exist_ok=True)
        assets.save_ply(os.path.join(a.terrain_dir, "map.ply"), verts, tris)
        assets.save_ply(os.path.join(a.terrain_dir, "big_stones.ply"), verts, rock_tris)
        print(f"mars seed {a.mars}: {plan.side}^2 nodes, {len(plan.hill_amp)} hills, {int(plan.stamp_kept.sum())} rocks, {len(rock_tris)} rock triangles")
    scene, uncovered, skipped = assets.generate_scene_files(eng, a.terrain_dir, n_cells=a.cells, res=a.res, k=a.k, horizontal_scale=a.hscale,
                                                            ranking=a.ranking)
    for sub, m in (("knn_terrain", scene.terrain), ("knn_rocks", scene.rocks)):
        print(f"{sub}: map_indices {tuple(m.map_indices.shape)}, {m.triangles.shape[0]} triangles, {m.vertices.shape[0]} vertices")
    print(f"heightmap_tensor.pt: {tuple(scene.heightmap.shape)} nodes at {a.hscale} m, {uncovered} uncovered, {skipped} triangles skipped")
    print(f"stone_info.npy: {scene.stone_info_raw.shape[0]} stones")
    print(f"done in {time.perf_counter() - t:.2f} s")
    if hasattr(eng, "close"):
        eng.close()
    return 0


if __name__ == "__main__":
    sys.exit(main())
