"""The entry points of rover_capi_scene.cpp: the KNN map builder, the heightfield rasteriser and the Mars terrain generator."""
import ctypes as C

import numpy as np
import torch

from ._abi import MARS_MAX_SIDE, MARS_TILE, EngineBase, MarsDesc, RoverError, _host, _ptr, host_call


def heightfield_limits():
    """rover_heightfield_limits: the sizes that separate the code paths of rover_build_heightfield as a dict — ``small_nodes``: the
    largest bounding box (nodes, clipped to the grid) one lane group rasterises; larger boxes are cut at the grid's multiples of
    ``tile_i`` x ``tile_j`` nodes, one workgroup per tile; ``group_lanes``: the lanes of a group.  Host only."""
    out = (C.c_int32 * 4)()
    host_call("rover_heightfield_limits", out)
    return {"small_nodes": int(out[0]), "tile_i": int(out[1]), "tile_j": int(out[2]), "group_lanes": int(out[3])}


def mars_desc(rows, cols, hill_window=(), hill_amp=(), g=(1.0,), class_tables=(), stamp_row=(), stamp_col=(), stamp_class=(), stamp_factor=(),
              stamp_kept=None):
    """A rover_mars_desc from host arrays -> (MarsDesc, the arrays it points into: keep them alive as long as the descriptor).
    ``hill_window`` [H, 6] (r0, r1, c0, c1, a0, b0), ``class_tables`` a sequence of square float64 arrays, ``stamp_kept`` defaults to
    all kept.  Nothing is checked here: the library does that."""
    win = np.ascontiguousarray(hill_window, dtype=np.int32).reshape(-1, 6)
    amp = np.ascontiguousarray(hill_amp, dtype=np.float64).reshape(-1)
    gg = np.ascontiguousarray(g, dtype=np.float64).reshape(-1)
    tabs = [np.ascontiguousarray(t, dtype=np.float64) for t in class_tables]
    side = np.asarray([t.shape[0] for t in tabs], dtype=np.int32)
    flat = np.concatenate([t.reshape(-1) for t in tabs]) if tabs else np.zeros(0, dtype=np.float64)
    sr, sc, sk = (np.ascontiguousarray(a, dtype=np.int32).reshape(-1) for a in (stamp_row, stamp_col, stamp_class))
    sf = np.ascontiguousarray(stamp_factor, dtype=np.float64).reshape(-1)
    kept = np.ones(len(sr), dtype=np.uint8) if stamp_kept is None else np.ascontiguousarray(np.asarray(stamp_kept) != 0, dtype=np.uint8).reshape(-1)
    if len(win) != len(amp) or not (len(sr) == len(sc) == len(sk) == len(sf) == len(kept)) or any(t.ndim != 2 or t.shape[0] != t.shape[1] for t in tabs):
        raise RoverError("mars_desc: hill arrays, stamp arrays or class tables of inconsistent shapes")
    ptr = lambda a: a.ctypes.data if a.size else None
    d = MarsDesc(int(rows), int(cols), len(amp), ptr(win), ptr(amp), ptr(gg), len(gg), len(tabs), ptr(side), ptr(flat), len(sr), ptr(sr), ptr(sc),
                 ptr(sk), ptr(sf), ptr(kept))
    return d, (win, amp, gg, side, flat, sr, sc, sk, sf, kept)


def mars_plan_desc(plan):
    """The rover_mars_desc of a ``terrain_gen.MarsPlan`` -> (MarsDesc, keep-alive)."""
    return mars_desc(plan.side, plan.side, plan.hill_windows(), plan.hill_amp, plan.g, plan.class_tables, plan.stamp_rows, plan.stamp_cols,
                     plan.stamp_class, plan.stamp_factor, plan.stamp_kept)


def mars_tiles(desc):
    """rover_mars_tiles: the per-tile stamp lists rover_mars_heightfield builds for ``desc`` (a MarsDesc) -> (tile_start [tiles + 1],
    tile_items) int32 arrays; tile (ti, tj) of MARS_TILE^2 nodes has the number ti ceil(cols / MARS_TILE) + tj.  Host only."""
    n = C.c_int64()
    host_call("rover_mars_tiles", C.byref(desc), None, None, 0, C.byref(n))
    tiles = ((desc.rows + MARS_TILE - 1) // MARS_TILE) * ((desc.cols + MARS_TILE - 1) // MARS_TILE)
    start, items = np.zeros(tiles + 1, dtype=np.int32), np.zeros(max(n.value, 1), dtype=np.int32)
    host_call("rover_mars_tiles", C.byref(desc), start.ctypes.data, items.ctypes.data, n.value, C.byref(n))
    return start, items[:n.value]


class SceneEngine(EngineBase):
    def build_knn_map(self, vertices, triangles, n_x, n_y, res=0.1, k=200, ranking="exact_f32", cell_x_f16=None, cell_y_f16=None):
        """rover_utils.py:48-123 on the GPU: -> map_indices [X, Y, K] int32 (device tensor), nearest first.
        ``ranking``: "exact_f32" (exact f32 squared distance, ties by id) or "reference_fp16" (the reference's fp16 distances,
        rover_utils.py:71-102; ``cell_*_f16`` = optional fp16 coordinate tables, see rover_build_knn_map_ref)."""
        v = _host(vertices, np.float32)
        t = _host(triangles, np.int32)
        if v.ndim != 2 or v.shape[1] != 3 or t.ndim != 2 or t.shape[1] != 3:
            raise RoverError("build_knn_map: expected vertices [V,3] and triangles [T,3]")
        out = torch.empty(int(n_x), int(n_y), int(k), dtype=torch.int32, device=self.device)
        mesh = (v.ctypes.data, v.shape[0], t.ctypes.data, t.shape[0], int(n_x), int(n_y), float(res), int(k))
        if ranking == "exact_f32":
            self._call("rover_build_knn_map", *mesh, _ptr(out))
            return out
        if ranking != "reference_fp16":
            raise RoverError(f"build_knn_map: unknown ranking {ranking!r}")
        tabs = []
        for tab, n in ((cell_x_f16, n_x), (cell_y_f16, n_y)):
            if tab is None:
                tabs.append(None)
                continue
            a = np.ascontiguousarray(np.asarray(tab, dtype=np.float16)).view(np.uint16)
            if a.shape != (int(n),):
                raise RoverError(f"build_knn_map: fp16 cell table must have {n} entries")
            tabs.append(a)
        self._call("rover_build_knn_map_ref", *mesh, *[None if a is None else a.ctypes.data for a in tabs], _ptr(out))
        return out

    def build_heightfield(self, vertices, triangles, n0, n1, horizontal_scale=0.025, shift=(0.0, 0.0), fill=0.0):
        """rover_build_heightfield: for every node (i, j) of an ``n0`` x ``n1`` grid at ``horizontal_scale`` metres, node (0, 0) at
        ``shift``, the highest point of the mesh above it (the definition is in include/rover_step.h) -> (hm [n0, n1] float32 device
        tensor in metres, nodes no triangle covers — they hold ``fill`` —, triangles skipped).  ``vertices`` [V, 3] / ``triangles`` [T, 3]:
        anything numpy understands, or torch tensors; float32 / int32 contiguous tensors on this device are passed as they are."""
        def arg(a, np_dtype, t_dtype):
            if isinstance(a, torch.Tensor) and a.is_cuda and a.device == self.device and a.dtype == t_dtype and a.is_contiguous():
                return a, a.data_ptr(), tuple(a.shape)
            h = _host(a, np_dtype)
            return h, h.ctypes.data, h.shape
        v, v_ptr, v_shape = arg(vertices, np.float32, torch.float32)
        t, t_ptr, t_shape = arg(triangles, np.int32, torch.int32)
        if len(v_shape) != 2 or v_shape[1] != 3 or len(t_shape) != 2 or t_shape[1] != 3:
            raise RoverError("build_heightfield: expected vertices [V,3] and triangles [T,3]")
        n0, n1 = int(n0), int(n1)
        out = torch.empty(max(n0, 0), max(n1, 0), dtype=torch.float32, device=self.device) if max(n0, n1) <= 131072 else None
        stats = (C.c_int64 * 2)()
        self._call("rover_build_heightfield", v_ptr if v_shape[0] else None, v_shape[0], t_ptr if t_shape[0] else None, t_shape[0], n0, n1,
                   float(horizontal_scale), float(shift[0]), float(shift[1]), float(fill), _ptr(out) if out is not None and out.numel() else None,
                   stats)
        return out, int(stats[0]), int(stats[1])

    def mars_heightfield(self, plan, rock_mask=True):
        """rover_mars_heightfield: the heightfield of the reference's Mars terrain generator from ``plan`` — a ``terrain_gen.MarsPlan``, or a
        ``MarsDesc`` (mars_desc: any rectangle) -> (hf [rows, cols] float64 device tensor in metres, rock_mask uint8 device tensor: 1 where
        a kept stamp covers the node; None with ``rock_mask=False``).  The definition is in include/rover_step.h; synchronous."""
        desc, keep = (plan, None) if isinstance(plan, MarsDesc) else mars_plan_desc(plan)
        ok = 1 <= desc.rows <= MARS_MAX_SIDE and 1 <= desc.cols <= MARS_MAX_SIDE
        hf = torch.empty(desc.rows, desc.cols, dtype=torch.float64, device=self.device) if ok else None
        mask = torch.empty(desc.rows, desc.cols, dtype=torch.uint8, device=self.device) if ok and rock_mask else None
        self._call("rover_mars_heightfield", C.byref(desc), _ptr(hf), _ptr(mask))
        del keep
        return hf, mask
