#!/usr/bin/env python
"""Writes tests/golden/mars_*.npz: what the reference's own terrain generator (omniisaacgymenvs/utils/terrain_utils/terrain_generation.py)
produces, recorded as data, next to the MarsPlan with which tests/mars_ref.py reproduces it.

  python tools/gen_mars_golden.py --reference /path/to/reference/checkout

Needs scipy (the reference's Halton sampler) and is run by hand; no test imports it.  The reference's module is imported with a stub
``pymeshlab``, without writing bytecode next to it, and with ``torch.empty(..., device="cuda:0")`` coerced to the CPU.  Recorded per case:
the Halton integers of the hills and of the rocks, every ``random.uniform`` / ``random.random`` draw in call order, the final float64
heightfield, ``rocks``, and for case A the mesh with slope_threshold None and 1.5.
"""
import argparse
import importlib.util
import os
import random
import sys
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

CASES = {    # name: width, horizontal_scale, kernel_radius, seed
    "A": (12.8, 0.1, 3.0, 10),
    "B": (12.8, 0.05, 3.0, 10),
    "C": (6.4, 0.025, 1.5, 10),
    "D": (12.8, 0.1, 3.0, 4242),
}
MAX_HEIGHT = 1.0


def load_reference(root):
    sys.dont_write_bytecode = True
    sys.modules.setdefault("pymeshlab", types.ModuleType("pymeshlab"))
    path = os.path.join(root, "omniisaacgymenvs", "utils", "terrain_utils", "terrain_generation.py")
    spec = importlib.util.spec_from_file_location("reference_terrain_generation", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    mod.torch = types.SimpleNamespace(empty=lambda *a, device=None, **k: torch.empty(*a, **k), cat=torch.cat)
    return mod


def run_reference(mod, width, hs, radius, seed):
    """-> dict of the recorded outputs.  The module's ``random`` and ``qmc`` are wrapped for the run and restored after it."""
    draws, halton = [], []
    real_uniform, real_random, real_seed, real_qmc = random.uniform, random.random, random.seed, mod.qmc

    def uniform(a, b):
        v = real_uniform(a, b)
        draws.append(v)
        return v

    def rand():
        v = real_random()
        draws.append(v)
        return v

    class Halton(real_qmc.Halton):
        def random(self, n=1, **kw):
            out = super().random(n=n, **kw)
            halton.append(out)              # the caller scales and truncates this array in place before .astype(int)
            return out

    random.uniform, random.random = uniform, rand
    mod.qmc = types.SimpleNamespace(Halton=Halton)
    try:
        t = mod.SubTerrain1(width=width, length=width, vertical_scale=1.0, horizontal_scale=hs)
        if seed != 10:                      # the reference seeds with 10 itself: seed here and make its call a no-op
            random.seed(seed)
            random.seed = lambda *a, **k: None
        t = mod.gaussian_terrain(t, kernel_radius=radius, max_height=MAX_HEIGHT)
        t, rocks = mod.add_rocks_terrain(t)
    finally:
        random.uniform, random.random, random.seed, mod.qmc = real_uniform, real_random, real_seed, real_qmc
    cells = [h.astype(int) for h in halton]
    return {"ref_halton_hills": cells[0].astype(np.int64), "ref_halton_rocks": np.concatenate(cells[1:]).astype(np.int64).reshape(-1, 2),
            "ref_draws": np.asarray(draws, dtype=np.float64), "ref_hf": t.height_field_raw.copy(), "ref_rocks": rocks.numpy().copy()}


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--reference", required=True, help="a checkout of the reference project")
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden"))
    args = ap.parse_args(argv)
    from isaac_rover_amd import terrain_gen
    import mars_ref
    mod = load_reference(args.reference)
    for name, (width, hs, radius, seed) in CASES.items():
        rec = run_reference(mod, width, hs, radius, seed)
        plan = terrain_gen.plan_mars_terrain(width, hs, seed=seed, kernel_radius=radius, max_height=MAX_HEIGHT)
        hf, _ = mars_ref.apply_plan(plan)
        assert hf.shape == rec["ref_hf"].shape and rec["ref_hf"].dtype == np.float64
        same = np.array_equal(mars_ref.bits(hf), mars_ref.bits(rec["ref_hf"]))
        if not same or not np.array_equal(plan.rocks, rec["ref_rocks"]):
            raise SystemExit(f"case {name}: the plan does not reproduce the reference (heights equal: {same})")
        if name == "A":
            v0, tri = mod.convert_heightfield_to_trimesh1(rec["ref_hf"], hs, 1.0, None)
            v1, _ = mod.convert_heightfield_to_trimesh1(rec["ref_hf"], hs, 1.0, 1.5)
            assert not np.array_equal(v0, v1), "the slope threshold moved no vertex"
            rec.update(ref_mesh_vertices=v0, ref_mesh_vertices_slope=v1, ref_mesh_triangles=tri.astype(np.int32))
        per_class = np.bincount(plan.stamp_class, minlength=len(plan.class_side)).tolist()
        path = os.path.join(args.out, f"mars_{name}.npz")
        plan.save(path, width=width, kernel_radius=radius, seed=seed, max_height=MAX_HEIGHT, **rec)
        print(f"{name}: {hf.shape[0]}^2 nodes, {len(plan.hill_amp)} hills, stamps per class {per_class}, kept {int(plan.stamp_kept.sum())} of "
              f"{len(plan.stamp_kept)}, {len(rec['ref_draws'])} draws, {os.path.getsize(path)} bytes")
    return 0


if __name__ == "__main__":
    sys.exit(main())
