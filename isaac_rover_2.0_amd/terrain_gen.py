"""The reference's Mars terrain generator (omniisaacgymenvs/utils/terrain_utils/terrain_generation.py) as a plan plus a mesh converter.

``plan_mars_terrain`` decides, on the host, everything ``gaussian_terrain`` (:104-153) and ``add_rocks_terrain`` (:18-65) decide before
they touch the heightfield: where the Gaussian hills and the rock stamps go, their tables and their random factors.  Applying the plan is
``Engine.mars_heightfield`` (rover_mars_heightfield, csrc/rover_mars.hip); tests/mars_ref.py applies it with numpy.
``heightfield_to_trimesh`` is ``convert_heightfield_to_trimesh1`` (:155-215) in vectorised numpy.  No scipy, no pymeshlab.
"""
from __future__ import annotations

import math
import random
from dataclasses import dataclass, fields

import numpy as np

MAX_HORIZONTAL_SCALE = 0.1          # above it the reference's own rock stamping fails (a broadcast ValueError, seen at 0.2)


def radical_inverse(index, base: int) -> np.ndarray:
    """The van der Corput value of every ``index`` (int64 array) in ``base``, accumulated in float64 the way scipy's unscrambled Halton
    sampler does: digit by digit from the lowest, ``sum += digit * w`` with ``w`` starting at 1 / base and DIVIDED by base each round
    (base 3 rounds there, so exact rational arithmetic gives other integers after scaling)."""
    q = np.asarray(index, dtype=np.int64).copy()
    out = np.zeros(q.shape, dtype=np.float64)
    w = 1.0 / base
    while q.size and int(q.max()) > 0:
        digit = q % base
        out += digit * w                                   # a finished index adds 0 * w = +0.0: no change
        w /= base
        q = (q - digit) // base
    return out


def halton_cells(first: int, count: int, n_rows: int, n_cols: int) -> np.ndarray:
    """Halton points ``first .. first + count - 1`` (bases 2 and 3, unscrambled), scaled by the field's sides and truncated -> [count, 2]
    int64: what ``(sampler.random(n) * (num_rows, num_cols)).astype(int)`` yields for a sampler that has already produced ``first``."""
    idx = np.arange(first, first + count, dtype=np.int64)
    return np.stack([(radical_inverse(idx, 2) * n_rows).astype(np.int64), (radical_inverse(idx, 3) * n_cols).astype(np.int64)], axis=1)


def gaussian_samples(n_samples, sigma, normalized: bool) -> np.ndarray:
    """``gaussian_distribution`` (:79-95): the normal density at the points np.arange makes of [-1, 1] in steps of 2 / (n_samples - 1)
    (``n_samples`` may be a float, as the hills pass it), optionally mapped onto [0, 1]."""
    step = 2 / (n_samples - 1)
    xs = np.arange(-1, 1 + 1e-7, step)
    v = np.asarray([(1 / (sigma * math.sqrt(2 * math.pi))) * math.exp(-0.5 * (x / sigma) * (x / sigma)) for x in xs], dtype=np.float64)
    if normalized:
        v = (v - np.min(v)) / (np.max(v) - np.min(v))
    return v


def rock_table(size_class: int, scale: int, height: float, centre_fix: bool = True) -> np.ndarray:
    """The stamp of rock size class ``size_class`` (:43-49) -> [side, side] float64, side = 1 + size_class * scale: the sigma = 1 kernel
    scaled to a maximum of 1, its centre lowered to the value above it where that is below 1 (``centre_fix``: the reference's :45-46),
    times ``height`` and the sigmoid factor 2 / (1 + exp(-0.3 (side - 1)))."""
    side = 1 + size_class * scale
    d = gaussian_samples(side, 1, False)
    k = np.outer(d, d)
    k = k / np.max(k)
    c = int(side / 2)
    if centre_fix and k[c - 1, c] < 1:
        k[c, c] = k[c - 1, c]
    return np.multiply(np.ones((side, side)) * height, (k / np.max(k)) * (1 / (1 + np.exp(-size_class * scale * 0.3))) * 2)


def rock_area_law(cover: float, diameter: float) -> float:
    """``cfa`` (:10-16): the fraction of the area covered by rocks larger than ``diameter`` where rocks cover ``cover`` in all."""
    return cover * math.exp(-(1.79 + (0.152 / cover)) * diameter)


@dataclass
class MarsPlan:
    side: int                       # nodes per side of the square field
    horizontal_scale: float
    hill_diameter: float            # 2 R / hs + 1, a float as in the reference
    hill_rows: np.ndarray           # [H] int64  Halton column 0 x side (the reference's "x": it indexes AXIS 1 of the field)
    hill_cols: np.ndarray           # [H] int64  Halton column 1 x side (axis 0)
    hill_amp: np.ndarray            # [H] float64
    g: np.ndarray                   # [G] float64 the normalised 1-D hill table: a hill adds (g[a] g[b]) amp
    class_side: np.ndarray          # [Cl] int32
    class_tables: list              # Cl arrays [side, side] float64
    stamp_rows: np.ndarray          # [S] int64 first row (axis 0) of the stamp's square
    stamp_cols: np.ndarray          # [S] int64 first column
    stamp_class: np.ndarray         # [S] int32 index into class_tables
    stamp_factor: np.ndarray        # [S] float64
    stamp_kept: np.ndarray          # [S] bool: False where the square overruns the field (the draw is consumed all the same)
    rocks: np.ndarray               # [n_kept, 4] float32 (row hs + r, col hs + r, 0, r)

    def save(self, path: str, **extra) -> None:
        d = {f.name: getattr(self, f.name) for f in fields(self) if f.name != "class_tables"}
        d.update({f"class_table_{i}": t for i, t in enumerate(self.class_tables)})
        d.update(extra)
        np.savez_compressed(path, **d)

    @classmethod
    def load(cls, path, prefix: str = "") -> "MarsPlan":
        z = path if isinstance(path, np.lib.npyio.NpzFile) else np.load(path)
        kw = {}
        for f in fields(cls):
            if f.name == "class_tables":
                continue
            v = z[prefix + f.name]
            kw[f.name] = v.item() if v.ndim == 0 else v
        kw["class_tables"] = [z[f"{prefix}class_table_{i}"] for i in range(len(kw["class_side"]))]
        kw["side"] = int(kw["side"])
        return cls(**kw)

    def hill_windows(self) -> np.ndarray:
        """Per hill the clipped slices of :135-143 -> [H, 6] int32 (r0, r1, c0, c1, a0, b0): rows r0 .. r1 - 1 and columns c0 .. c1 - 1 of
        the field receive g[a0 + r - r0] g[b0 + c - c0] amp.  As in the reference the kernel's upper bound is diameter - 1, so its last
        row and column are never used, and Halton column 1 places axis 0."""
        n, kd = self.side, self.hill_diameter
        half = (kd - 1) / 2
        out = np.zeros((len(self.hill_amp), 6), dtype=np.int32)

        def axis(p):
            lo = p - half
            f0, f1 = int(max(0, lo)), int(min(n, p + half))
            k0, k1 = int(abs(min(0, lo))), int(abs(min(kd - 1, n - lo)))
            if f1 - f0 != k1 - k0 or k1 > len(self.g):
                raise ValueError(f"hill at {p}: the field slice {f0}:{f1} and the table slice {k0}:{k1} differ in length")
            return f0, f1, k0

        for i, (px, py) in enumerate(zip(self.hill_rows, self.hill_cols)):
            r0, r1, a0 = axis(py)
            c0, c1, b0 = axis(px)
            out[i] = (r0, r1, c0, c1, a0, b0)
        return out


def plan_mars_terrain(width, horizontal_scale, seed=10, kernel_radius=15.0, max_height=5.0, rock_cover=0.03, rock_height=(0.1, 0.2)) -> MarsPlan:
    """The plan of ``gaussian_terrain(t, kernel_radius, max_height); add_rocks_terrain(t, rock_height)`` on a square
    ``SubTerrain1(width=width, length=width, horizontal_scale=horizontal_scale, vertical_scale=1)``.  One ``random.Random(seed)`` serves
    the hills and then the rocks; seed 10 is the reference's own (``gaussian_terrain`` seeds the module's generator with 10 and
    ``add_rocks_terrain`` continues it).  ``rock_cover`` is the reference's constant k = 0.03."""
    hs = float(horizontal_scale)
    if not (width > 0) or not (hs > 0) or not math.isfinite(width):
        raise ValueError(f"plan_mars_terrain: width = {width} and horizontal_scale = {horizontal_scale} must be positive")
    if hs > MAX_HORIZONTAL_SCALE:
        raise ValueError(f"plan_mars_terrain: horizontal_scale = {hs} is above {MAX_HORIZONTAL_SCALE} (the reference's rock stamping fails there)")
    n = int(width / hs)
    if n < 1:
        raise ValueError(f"plan_mars_terrain: width = {width} holds no node at horizontal_scale = {hs}")
    rng = random.Random(seed)

    # hills (:111-149)
    kd = ((2 * kernel_radius) / hs) + 1
    g = gaussian_samples(kd, 0.4, True)
    n_hills = int((width / (kernel_radius * 2)) * (width / (kernel_radius * 2))) + 8
    cells = halton_cells(0, n_hills, n, n)
    amp = np.asarray([rng.uniform(-max_height, max_height) for _ in range(n_hills)], dtype=np.float64)

    # rocks (:20-63): one Halton sequence runs on through the size classes
    step = max(0.10, hs)
    scale = int(step / hs)
    sides, tables, rows, cols, cls, factor, kept, rocks = [], [], [], [], [], [], [], []
    produced = 0
    for ci, i in enumerate(range(1, int(0.5 / step))):
        radius = (i * step) / 2
        lower = width * width * rock_area_law(rock_cover, i * step)
        upper = width * width * rock_area_law(rock_cover, (i + 1) * step)
        count = max(int((lower - upper) / (radius * radius * 3.1415)), 0)
        pos = halton_cells(produced, count, n, n)
        produced += count
        table = rock_table(i, scale, rng.uniform(rock_height[0], rock_height[1]))
        side = table.shape[0]
        sides.append(side)
        tables.append(table)
        for r, c in pos:
            f = rng.random() * 0.4 + 0.6                   # drawn before the reference's += fails on a clipped slice
            ok = bool(r + side <= n and c + side <= n)
            rows.append(int(r)); cols.append(int(c)); cls.append(ci); factor.append(f); kept.append(ok)
            if ok:
                rocks.append((r * hs + radius, c * hs + radius, 0, radius))
    plan = MarsPlan(side=n, horizontal_scale=hs, hill_diameter=float(kd), hill_rows=cells[:, 0].copy(), hill_cols=cells[:, 1].copy(), hill_amp=amp, g=g,
                    class_side=np.asarray(sides, dtype=np.int32), class_tables=tables, stamp_rows=np.asarray(rows, dtype=np.int64),
                    stamp_cols=np.asarray(cols, dtype=np.int64), stamp_class=np.asarray(cls, dtype=np.int32),
                    stamp_factor=np.asarray(factor, dtype=np.float64), stamp_kept=np.asarray(kept, dtype=bool),
                    rocks=np.asarray(rocks, dtype=np.float64).reshape(-1, 4).astype(np.float32))
    plan.hill_windows()                                    # raises where the reference's hill slices would not broadcast
    return plan


def grid_triangles(n_rows: int, n_cols: int) -> np.ndarray:
    """Two triangles per grid square, (v, v + n_cols + 1, v + 1) and (v, v + n_cols, v + n_cols + 1): the reference's :200-213 and the
    diagonal of ``synth.grid_mesh`` -> [2 (n_rows - 1)(n_cols - 1), 3] int32, row-major over the squares."""
    v = (np.arange(n_rows - 1, dtype=np.int64)[:, None] * n_cols + np.arange(n_cols - 1, dtype=np.int64)[None, :]).reshape(-1)
    t = np.empty((len(v), 2, 3), dtype=np.int64)
    t[:, 0] = np.stack([v, v + n_cols + 1, v + 1], axis=1)
    t[:, 1] = np.stack([v, v + n_cols, v + n_cols + 1], axis=1)
    return t.reshape(-1, 3).astype(np.int32)


def heightfield_to_trimesh(hf, horizontal_scale, slope_threshold=None):
    """``convert_heightfield_to_trimesh1`` (:155-215) at vertical_scale 1 -> (vertices [R C, 3] float32, triangles int32).  Vertex
    (i, j) sits at (i hs, j hs, hf[i, j]); with ``slope_threshold`` a vertex at the foot of a step steeper than it moves one node spacing
    towards the step, per axis and along the diagonal, as the reference does."""
    hf = np.asarray(hf, dtype=np.float64)
    n_rows, n_cols = hf.shape
    hs = horizontal_scale
    y = np.linspace(0, (n_cols - 1) * hs, n_cols)
    x = np.linspace(0, (n_rows - 1) * hs, n_rows)
    yy, xx = np.meshgrid(y, x)
    if slope_threshold is not None:
        thr = slope_threshold * hs
        move_x = np.zeros((n_rows, n_cols))
        move_y = np.zeros((n_rows, n_cols))
        move_c = np.zeros((n_rows, n_cols))
        move_x[:-1, :] += (hf[1:, :] - hf[:-1, :] > thr)
        move_x[1:, :] -= (hf[:-1, :] - hf[1:, :] > thr)
        move_y[:, :-1] += (hf[:, 1:] - hf[:, :-1] > thr)
        move_y[:, 1:] -= (hf[:, :-1] - hf[:, 1:] > thr)
        move_c[:-1, :-1] += (hf[1:, 1:] - hf[:-1, :-1] > thr)
        move_c[1:, 1:] -= (hf[:-1, :-1] - hf[1:, 1:] > thr)
        xx = xx + (move_x + move_c * (move_x == 0)) * hs
        yy = yy + (move_y + move_c * (move_y == 0)) * hs
    vertices = np.zeros((n_rows * n_cols, 3), dtype=np.float32)
    vertices[:, 0] = xx.reshape(-1)
    vertices[:, 1] = yy.reshape(-1)
    vertices[:, 2] = hf.reshape(-1)
    return vertices, grid_triangles(n_rows, n_cols)
