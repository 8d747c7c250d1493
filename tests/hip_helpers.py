"""Helpers for the -m gpu parity tests: drive the HIP path through the C ABI (isaac_rover_amd._lib)."""
import numpy as np
import torch

from isaac_rover_amd import _lib

EXTRA_DT = {k: (torch.int64 if k == "collision_penalty" else torch.float32) for k in _lib.EXTRAS}


def make_engine(scene, distribution, num_envs, variant=3, run=None, **kw):
    """``variant`` defaults to the culled ray cast (the kernel full batches run; the library itself falls back to the binned
    kernel 2 for the as-shipped fp16 maths): at test sizes the library's auto choice would be the env-order kernel.
    None = leave the auto choice."""
    eng = _lib.Engine(num_envs, device=0, **kw)
    eng.set_scene(scene, distribution)
    if variant is not None:
        eng.set_option("raycast_variant", variant)
    if run is not None:
        eng.set_option("raycast_run", run)
    return eng


def hip_step(eng, st, compact=True, fused=True, stone_margin=None):
    """One post_physics_step on the GPU. Returns a dict of CPU numpy arrays named like the oracle's.
    ``stone_margin``: also request the stone_info occupancy mask (BASELINE configs[2]) -> out["stone_collision"]."""
    dev = eng.device
    e = eng.num_envs
    d = {k: v.to(dev).contiguous() for k, v in st.items()}
    progress = d["progress"].clone()
    sin = eng.make_in(d["pos"], d["quat"], d["joints"], d["target"], d["lin_hist"], d["ang_hist"], d["euler_pre"], progress)
    f, i64 = torch.float32, torch.int64
    obs = torch.zeros(e, eng.num_observations, device=dev)
    bufs = dict(rew=torch.zeros(e, device=dev), reset=torch.ones(e, dtype=i64, device=dev),
                rock_collision=torch.zeros(e, dtype=i64, device=dev),
                reset_ids=torch.full((e,), -1, dtype=i64, device=dev), n_reset=torch.zeros(1, dtype=torch.int32, device=dev),
                euler=torch.zeros(e, 3, device=dev), heading_diff=torch.zeros(e, device=dev),
                ray_dist=torch.zeros(e, eng.P, device=dev), wheel_dist=torch.zeros(e, 24, device=dev),
                body_dist=torch.zeros(e, 2, device=dev))
    extras = {k: torch.zeros(e, dtype=EXTRA_DT[k], device=dev) for k in _lib.EXTRAS}
    done_u8 = torch.full((e,), 7, dtype=torch.uint8, device=dev)
    stone = None if stone_margin is None else torch.full((e,), -1, dtype=i64, device=dev)
    sout = eng.make_out(obs, extras=extras, done_u8=done_u8, stone_collision=stone, stone_margin=stone_margin or 0.0, **bufs)
    if fused:
        eng.step(sin, sout, increment_progress=True, compact=compact)
    else:   # the reference's method split, rl_task.py:250-257
        progress += 1
        eng.get_observations(sin, sout)
        eng.calculate_metrics(sin, sout)
        eng.is_done(sin, sout)
        if compact:
            eng.compact_resets(bufs["reset"], bufs["reset_ids"], bufs["n_reset"])
    torch.cuda.synchronize()
    out = dict(euler=bufs["euler"], heading_diff=bufs["heading_diff"], ray_dist=bufs["ray_dist"],
               wheel_dist=bufs["wheel_dist"], body_dist=bufs["body_dist"], rock_collision=bufs["rock_collision"],
               obs_buf=obs, rew_buf=bufs["rew"], reset_buf=bufs["reset"], progress_buf=progress)
    for k in _lib.EXTRAS:
        out["extras_" + k] = extras[k]
    if fused or True:
        out["done_u8"] = done_u8
    if stone is not None:
        out["stone_collision"] = stone
    out = {k: v.cpu().numpy() for k, v in out.items()}
    n = int(bufs["n_reset"].item())
    out["reset_ids"] = bufs["reset_ids"][:n].cpu().numpy()
    return out


def _oracle_maps(scene):
    from oracle import oracle as orc
    return (orc.KnnMap(scene.terrain.map_indices, scene.terrain.triangles, scene.terrain.vertices),
            orc.KnnMap(scene.rocks.map_indices, scene.rocks.triangles, scene.rocks.vertices))


def _rays_vs_oracle(eng, maps, half, label):
    """The ray phase on its own, free of the pose trigonometry: the device's OWN rays of the last step (origins and ray-record
    directions as prep_rays_kernel made them, `rover_export_rays`) through the oracle's per-ray arithmetic (ray_casting.py:34-59 + the
    cell lookup + min over K, `oracle.raycast_unit`) must give the device's distances bit for bit — every ray, both maps.
    -> (origins, cells, the oracle's distances [E][26 + P])"""
    from oracle import oracle as orc
    src, dirs, cell, dist = (x.cpu().numpy() for x in eng.export_rays())
    t, r = maps
    want_rock = orc.raycast_unit(r, src[:, :26], dirs[:, :26], half=half).reshape(dist[:, :26].shape)
    want_terr = orc.raycast_unit(t, src[:, 26:], dirs[:, 26:], half=half).reshape(dist[:, 26:].shape)
    # equal as IEEE values (a distance of exactly zero may come out as +0 from one triangle and -0 from another: which of the two equal
    # values a min returns is the reduction order's business — torch.min's too; 1 ray of 9.6 M at configs[4]), NaN where the oracle has NaN
    want_all = np.concatenate((want_rock, want_terr), axis=1)
    differ = ~((dist == want_all) | (np.isnan(dist) & np.isnan(want_all)))
    n_bad = int(differ.sum())
    n_bits = int((dist.view(np.uint32) != want_all.view(np.uint32)).sum())
    print(f"[{label}] ray phase on the device's own rays vs the oracle: {n_bad} of {dist.size} distances differ ({n_bits} in their bits: +0 / -0)")
    for e, sl in list(zip(*np.nonzero(differ)))[:8]:
        print(f"   env {e} slot {sl}: src {src[e, sl].tolist()} ({src[e, sl].view(np.uint32).tolist()}) dir {dirs[e, sl].tolist()} "
              f"({dirs[e, sl].view(np.uint32).tolist()}) cell {cell[e, sl]}: device {dist[e, sl]!r} oracle {want_all[e, sl]!r}")
    assert n_bad == 0, f"{label}: {n_bad} of {dist.size} ray distances differ from the oracle on IDENTICAL rays"
    return src, cell, want_all
