#!/usr/bin/env python3
"""CPU study (numpy) for the staged ray cast's level loop: the histogram of a heightmap ray's level L with the ray measured from its
ORIGIN (o = dist_xy(s, C), dzm = |s_z - z| over the suffix) and from the point s' where its line crosses the row's own height z_c
(`lane_rebase`), for the per-cell and the shared-row form of the tables.  EXPERIMENTS.md quotes its output.

The rows are restated from `ctab_build_kernel<0>` / `lane_build_kernel` (f32 proof, sphere records): padded triangle, smallest
enclosing sphere, cell-relative fp16 centre, r2' rounded up, G per pair, pairs ordered by G, a bound {G, z0, z1, rho_out, cone} per
suffix of 8 pairs, each rounded to fp16 on its safe side.  One shortcut: `ctab`'s r2 is taken as 1.06 rho^2 x 1.003 (the stored
normal's length overshoots `need` by 0.2-0.4 %).  The level loop is `lane_scan_kernel`'s, in float32.

    python tools/level_rebase_study.py [--cells 25] [--k 200] [--envs 4096] [--rays 37]
"""
import argparse
import math
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from isaac_rover_amd import synth  # noqa: E402
from oracle import torch_ref  # noqa: E402

f32 = np.float32
PAD, C_RHO, C_A, CONE_TAU, LN_PAD = 0.101, 1.06, 0.99925, 1.25e-2, 5.0e-5
LN_REB_ERR = 1.0e-6                      # rover_cull.hip: the rounding of s' per metre of |s_z - z_c|
CELL = 0.1


def far_consts():
    ca = C_A - 1.0e-5
    return f32(1.00001 / (0.9 * math.sqrt(ca))), f32(1.00001 * math.sqrt(1.00001 + 1.0e-5 - ca) / (0.9 * math.sqrt(ca)))


def h_down(v):
    h = np.asarray(v, dtype=np.float64).astype(np.float16)
    bad = np.isfinite(h) & (h.astype(np.float64) > v)
    return np.where(bad, np.nextafter(h, np.float16(-np.inf)), h).astype(np.float16)


def h_up(v):
    h = np.asarray(v, dtype=np.float64).astype(np.float16)
    bad = np.isfinite(h) & (h.astype(np.float64) < v)
    return np.where(bad, np.nextafter(h, np.float16(np.inf)), h).astype(np.float16)


def triangle_spheres(verts16, tris):
    """ctab_build_kernel<0>: centre (x, y in f32, z in fp16), rho + 1e-4, |N_z| / |N| per triangle."""
    v = verts16.astype(np.float32)[tris]                                     # [T, 3 corners, 3]
    a = v[:, 2].astype(np.float64)
    b = (v[:, 1] - v[:, 2]).astype(np.float64)
    c = (v[:, 0] - v[:, 2]).astype(np.float64)
    Q = np.stack([a - PAD * b - PAD * c, a + (1 + 2 * PAD) * b - PAD * c, a - PAD * b + (1 + 2 * PAD) * c], axis=1)
    d2 = lambda x, y: ((Q[:, x] - Q[:, y]) ** 2).sum(1)
    A, B, C = d2(1, 2), d2(0, 2), d2(0, 1)
    w = np.stack([A * (B + C - A), B * (C + A - B), C * (A + B - C)], axis=1)
    w /= w.sum(1, keepdims=True)
    w[A >= B + C] = (0.0, 0.5, 0.5)
    w[B >= A + C] = (0.5, 0.0, 0.5)
    w[C >= A + B] = (0.5, 0.5, 0.0)
    m = (w[:, :, None] * Q).sum(1)
    m[:, 0:2] = m[:, 0:2].astype(np.float32)
    m[:, 2] = m[:, 2].astype(np.float32).astype(np.float16)
    rho = np.sqrt(((Q - m[:, None, :]) ** 2).sum(2).max(1)) + 1.0e-4
    N = np.cross(b, c)
    return m, rho, np.abs(N[:, 2]) / np.linalg.norm(N, axis=1) * (1.0 - 1.0e-6)


def pair_up(ids):
    """idx4_build_kernel / lane_union_kernel: partners (2p, 2p + 1) that are both listed share a pair, the rest pair up in id order."""
    ids = np.unique(ids)
    have = set(int(t) for t in ids)
    firsts = [t for t in ids if not (t & 1) and (int(t) | 1) in have]
    singles = [t for t in ids if (int(t) ^ 1) not in have]
    pairs = [(t, t | 1) for t in firsts]
    pairs += [(singles[i], singles[i + 1] if i + 1 < len(singles) else -1) for i in range(0, len(singles), 2)]
    return np.asarray(pairs, dtype=np.int64)


def build_row(ids, C_xy, m, rho, nzq, k1):
    """lane_build_kernel: the 16 level records {Gq, z0, z1, rho_out, q16} of a row, and its z_c."""
    pairs = pair_up(ids)
    pp = ((len(pairs) + 7) // 8) * 8
    mz = m[ids, 2]
    zc = float(f32(0.5) * (f32(mz.min()) + f32(mz.max())))
    G = np.full(128, np.inf); z0 = np.full(128, np.inf); z1 = np.full(128, -np.inf); ro = np.zeros(128); qn = np.full(128, 2.0)
    for e in range(2):
        t = pairs[:, e]
        ok = t >= 0
        t = t[ok]
        f = (m[t] - np.array([C_xy[0], C_xy[1], zc])).astype(np.float32)
        h = f.astype(np.float16).astype(np.float64)
        enc = np.linalg.norm(np.array([C_xy[0], C_xy[1], zc]) + h - m[t], axis=1)
        r2c = C_RHO * rho[t] ** 2 * 1.003
        need = C_RHO * (np.sqrt(r2c / C_RHO) + enc + LN_PAD) ** 2 * 1.000001
        r2h = h_up(need * 1.0000001).astype(np.float32)
        hx, hy = h[:, 0].astype(np.float32), h[:, 1].astype(np.float32)
        dxy = np.sqrt(hx * hx + hy * hy, dtype=f32)
        g = (dxy - k1 * np.sqrt(r2h, dtype=f32) * f32(1.00001)) * f32(0.99999) - f32(1.0e-6)
        idx = np.nonzero(ok)[0]
        G[idx] = np.minimum(G[idx], g)
        z0[idx] = np.minimum(z0[idx], h[:, 2]); z1[idx] = np.maximum(z1[idx], h[:, 2])
        ro[idx] = np.maximum(ro[idx], dxy * f32(1.00001)); qn[idx] = np.minimum(qn[idx], nzq[t])
    order = np.argsort(G, kind="stable")
    G, z0, z1, ro, qn = G[order], z0[order], z1[order], ro[order], qn[order]
    lv = np.zeros((16, 5), dtype=np.float32)
    for k in range(16):
        s = slice(8 * k, 128)
        a0, a1 = z0[s].min(), z1[s].max()
        if not a0 <= a1:
            a0 = a1 = 0.0
        gq = h_down(float(f32(G[s].min()) * f32(0.9999) - f32(1.0e-5))) if 8 * k < pp else np.float16(-np.inf)
        q = qn[s].min()
        q16 = 0xfffe if q > 1.0 else min(0xfffe, int(math.floor(float(f32(q) * f32(65535.0)))) if q > 0 else 0)
        lv[k] = (float(gq), float(h_down(a0)), float(h_up(a1)), float(h_up(ro[s].max())), q16)
    return lv, zc, pp // 8


def levels(lv, nch, s, d, rq, k2, rebase):
    """lane_scan_kernel's level loop, vectorised over rays: s [n, 3] cell-relative origins (f32), d [n, 3] (f32), lv [n, 16, 5]."""
    sx, sy, sz = s[:, 0], s[:, 1], s[:, 2]
    dx, dy, dz = d[:, 0], d[:, 1], d[:, 2]
    dxy2 = dx * dx + dy * dy
    adz = np.abs(dz)
    sq = np.sqrt(dxy2, dtype=f32)
    steep = adz * adz >= f32(0.81) * (dxy2 + adz * adz) * f32(1.0001)
    c3 = k2 * adz * sq * f32(1.0004)
    c4 = (sq + k2 * adz * adz) * f32(1.0004)
    if rebase:
        tz = sz * (f32(1.0) / dz)
        lx, ly, lz = sx - tz * dx, sy - tz * dy, np.zeros_like(sz)
        kz = k2 * f32(1.0004 * 1.0021) + f32(LN_REB_ERR)
        extra = kz * np.abs(sz)
    else:
        lx, ly, lz, extra = sx, sy, sz, f32(0.0)
    o = np.sqrt(lx * lx + ly * ly, dtype=f32)
    base = -((adz * f32(1.0004) + c3) * o + extra)
    L = nch.copy()
    for k in range(15, -1, -1):
        Gq, z0, z1, ro, q16 = (lv[:, k, i] for i in range(5))
        dzm = np.maximum(np.abs(lz - z0), np.abs(lz - z1))
        lhs = Gq * adz + (ro * (-c3) + base)
        L = np.where((lhs > dzm * c4) & (q16 >= rq), k, L)
    return np.where(steep, L, nch)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cells", type=int, default=25)
    ap.add_argument("--k", type=int, default=200)
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--rays", default="37")
    ap.add_argument("--height", type=float, default=0.5, help="the rover's origin above the surface (make_states: 0.5)")
    args = ap.parse_args()
    n = args.cells
    scene = synth.make_scene(n_cells=n, k=args.k, n_stones=16)
    verts16 = scene.terrain.vertices.numpy()
    tris = scene.terrain.triangles.numpy().astype(np.int64)
    idx = scene.terrain.map_indices.numpy().astype(np.int64)
    m, rho, nzq = triangle_spheres(verts16, tris)
    k1, k2 = far_consts()

    # rays of make_states' poses (roll, pitch 0.1 rad sigma, origin + 0.5 m), as the oracle forms them; only those whose cell is their own
    # (a 2.5 m map: the outer rings of the 37-ray set leave it and are clamped into a border cell, where no level is ever cleared)
    st = synth.make_states(args.envs, n * CELL, seed=31, margin_m=0.3)
    st["pos"][:, 2] += args.height - 0.5
    pts = torch.as_tensor(synth.ray_distribution(args.rays)[0], dtype=torch.float64)
    p = pts.shape[0]
    eul = torch_ref._quat_to_euler(st["quat"].float())
    local = torch.cat((pts, torch.tensor([[0.0, 0.0, -1.0]], dtype=torch.float64)))[None].expand(args.envs, p + 1, 3)
    world = torch_ref._body_xf(local, eul, st["pos"].float())
    src = world[:, :p].float()
    dirs = (world[:, p:] - st["pos"].double()[:, None, :]).expand(args.envs, p, 3).float()
    dd = (-torch.nn.functional.normalize(dirs, dim=2)).reshape(-1, 3).numpy()
    ss = src.reshape(-1, 3).numpy()
    raw = ss[:, 0:2] / f32(CELL)
    inside = (raw[:, 0] >= -0.5) & (raw[:, 0] <= n - 0.5) & (raw[:, 1] >= -0.5) & (raw[:, 1] <= n - 0.5)
    ss, dd = ss[inside], dd[inside]
    ij = np.rint(np.clip(ss[:, 0:2] / f32(CELL), 0, n - 1)).astype(np.int64)
    qm = f32(CONE_TAU) * np.abs(dd[:, 2]) + np.sqrt(dd[:, 0] ** 2 + dd[:, 1] ** 2, dtype=f32) + f32(2.0e-5)
    rq = np.where(qm < f32(0.9999), np.ceil(qm * f32(65535.0)), 65535.0)
    print(f"scene {n} x {n} cells, K = {args.k}; {len(ss)} heightmap rays inside the map of {args.envs} x {p}; "
          f"origin {float(np.mean(ss[:, 2])):.2f} m mean z, tilt {float(np.mean(np.arccos(np.abs(dd[:, 2])))):.3f} rad mean")

    for form in ("per-cell rows", "shared rows"):
        shared = form == "shared rows"
        rows = {}
        used = set((int(a), int(b) // 2 * 2) for a, b in ij) if shared else set((int(a), int(b)) for a, b in ij)
        if shared:
            for x in range(n):
                for j in range(0, n, 2):
                    if (x, j) not in used:
                        continue
                    two = j + 1 < n
                    ids = np.concatenate([idx[x, j], idx[x, j + 1]]) if two else idx[x, j]
                    rows[(x, j // 2)] = build_row(ids, (f32(x) * f32(CELL), (f32(j) + f32(0.5)) * f32(CELL) if two else f32(j) * f32(CELL)), m, rho, nzq, k1) + \
                        ((float(f32(x) * f32(CELL)), float((f32(j) + f32(0.5)) * f32(CELL) if two else f32(j) * f32(CELL))),)
            key = [(int(a), int(b) // 2) for a, b in ij]
        else:
            for x in range(n):
                for y in range(n):
                    if (x, y) not in used:
                        continue
                    rows[(x, y)] = build_row(idx[x, y], (f32(x) * f32(CELL), f32(y) * f32(CELL)), m, rho, nzq, k1) + \
                        ((float(f32(x) * f32(CELL)), float(f32(y) * f32(CELL))),)
            key = [(int(a), int(b)) for a, b in ij]
        lv = np.stack([rows[k][0] for k in key])
        zc = np.array([rows[k][1] for k in key], dtype=np.float32)
        nch = np.array([rows[k][2] for k in key], dtype=np.int64)
        cxy = np.array([rows[k][3] for k in key], dtype=np.float32)
        s_rel = np.stack([ss[:, 0] - cxy[:, 0], ss[:, 1] - cxy[:, 1], ss[:, 2] - zc], axis=1).astype(np.float32)
        for rebase in (False, True):
            L = levels(lv, nch, s_rel, dd.astype(np.float32), rq, k2, rebase)
            hist = [np.mean(L <= 1), np.mean(L == 2), np.mean(L == 3), np.mean(L == 4), np.mean(L == 5), np.mean((L == 6) | (L == 7)), np.mean(L >= 8)]
            print(f"{form:14s} {'from s_prime' if rebase else 'from origin '}: mean L {L.mean():.3f}   L <=1 / 2 / 3 / 4 / 5 / 6-7 / >=8 = "
                  + " / ".join(f"{100 * h:.1f}" for h in hist) + " %")


if __name__ == "__main__":
    main()
