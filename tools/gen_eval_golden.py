"""TEST INFRASTRUCTURE — generates tests/golden/eval_seq_e64_p37_{fp32,fp16_as_shipped}.npz from the reference's own
evaluation branch (rover.py:122-137 buffers, :620-641 is_done, :670-672 check_collision).

Run in the build container only (needs the reference next to oracle/ref_harness.py):

    PYTHONDONTWRITEBYTECODE=1 python tools/gen_eval_golden.py

A fixture is a sequence of T scripted steps over E envs on the step fixtures' synthetic scene: per step the sim state fed to the
reference (``in_*`` [T, E, ...]), the curriculum level and global step it ran at, and what it produced (``out_rock_collision``,
``out_reset_buf``, ``out_progress_buf``, ``out_eval_res`` [T, E]).  ``rover_eval_res`` is carried from one step to the next like the
task's buffer.  The reference's ``get_observations`` / ``calculate_metrics`` / ``is_done`` are called unbound in rl_task order on the
namespace of ``oracle.ref_harness.Reference.make_task`` with ``is_evaluation = True``; each step runs in a scratch working directory so
that the files its save step writes (:632-640) are read back into the fixture (``save_*``).
"""
from __future__ import annotations

import contextlib
import io
import os
import sys
import tempfile

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from isaac_rover_amd import synth  # noqa: E402
from oracle import gen_golden as gg  # noqa: E402
from oracle import ref_harness as rh  # noqa: E402

E, T = 64, 10
LEVEL = [1, 1, 1, 2, 2, 2, 2, 2, 2, 2]          # a stretch at level 1 (no collision latch), then level 2
GLOBAL_STEP0 = 2995                              # global_step of step k is 2995 + k: step 5 is a save step (3000 % 3000 == 0)
NAME = "rover_eval_no_noise_teacher_rocks_small_area_removedv5"   # self._name after the first pre_physics_step (rover.py:376)
F = np.float32
X0 = 0.03125                                     # the scripted rovers' column (clear of the rocks from y = 6 to 9.5); X0 + td is exact in f32


def up(x):
    return float(np.nextafter(F(x), F(np.inf)))


def down(x):
    return float(np.nextafter(F(x), F(-np.inf)))


def scripted_states(scene):
    """T per-step copies of one random batch; the rovers drift between steps, and envs 0..14 are scripted (see the table below)."""
    base = synth.make_states(E, gg.SCENE_KW["n_cells"] * 0.1, seed=31)
    g = torch.Generator().manual_seed(77)
    ang = 2 * np.pi * torch.rand(E, generator=g)
    drift = torch.stack((torch.cos(ang), torch.sin(ang)), 1) * 0.05
    info = synth.read_stone_info_array(scene.stone_info_raw)
    inside = [i for i in range(info.shape[0]) if 1.5 < info[i, 0] < 11.3 and 1.5 < info[i, 1] < 11.3]

    def on_stone(st, e, n):
        s_ = info[inside[n]]
        st["pos"][e, 0], st["pos"][e, 1] = float(s_[0]), float(s_[1])
        i, j = float(s_[0]) / 0.1, float(s_[1]) / 0.1
        st["pos"][e, 2] = float(synth.surface_height(np.float64(i), np.float64(j))) + 0.3

    def place(st, e, x, y, td_x):
        """rover at (x, y), goal td_x metres along +x (x + td_x is an exact f32 sum here: the difference is exactly td_x)."""
        st["pos"][e, 0], st["pos"][e, 1] = x, y
        st["pos"][e, 2] = float(synth.surface_height(np.float64(x / 0.1), np.float64(y / 0.1))) + 0.5
        st["target"][e, 0] = float(F(x) + F(td_x))
        st["target"][e, 1] = y

    seq = []
    for k in range(T):
        st = {key: v.clone() for key, v in base.items()}
        st["pos"][:, 0:2] += k * drift
        st["progress"] = base["progress"] + k
        # goal at td = 0.18 exactly (e0) and 0.18 +- 1 ulp (e1); e0 then meets out of area (td = 10) and keeps its code 2
        place(st, 0, X0, 6.0, 0.18 if k >= 2 else 8.0)
        if k >= 6:
            place(st, 0, X0, 6.0, 10.0)
        place(st, 1, X0, 6.5, {2: up(0.18), 3: down(0.18)}.get(k, 8.0))
        # out of area at td = 9.5 (e2) and 9.5 -+ 1 ulp (e3), an env that stays between 9.5 and 11 (e4), the d >= 11 reset (e5)
        place(st, 2, X0, 7.0, 9.5 if k == 1 else 8.0)
        place(st, 3, X0, 7.5, down(9.5) if 1 <= k <= 3 else (up(9.5) if k == 4 else 8.0))
        place(st, 4, X0, 8.0, 10.0)
        place(st, 5, X0, 8.5, 11.5 if k == 2 else 8.0)
        # timeout: progress 2999 -> 3000 at step 1 (e6)
        st["progress"][6] = 2998 + k
        place(st, 6, X0, 9.0, 8.0)
        # tilt reset at step 1 (no code), then the goal at step 7 (e7)
        place(st, 7, X0, 9.5, 0.1 if k == 7 else 8.0)
        if k == 1:
            st["euler_pre"][7, 0] = 1.2
        # parked on a stone: no latch at level 1, code 1 from the first level-2 step (e8, e9)
        on_stone(st, 8, 4)
        on_stone(st, 9, 1)
        st["target"][8:10, 0:2] = st["pos"][8:10, 0:2] + torch.tensor([5.0, 0.0])
        # collision and goal in the same step (level 2): the collision wins (e10, on its stone from step 4 on)
        place(st, 10, X0, 6.25, 8.0)
        if k >= 4:
            on_stone(st, 10, 1)
            st["target"][10, 0:2] = st["pos"][10, 0:2] + torch.tensor([0.1, 0.05])
        # on a stone with its goal beside it at level 1: the goal latches, the collision does not (e11)
        on_stone(st, 11, 3)
        st["target"][11, 0:2] = st["pos"][11, 0:2] + torch.tensor([0.1, 0.05])
        # tilt and out of area in the same step: code 1 from the distance (e12)
        place(st, 12, X0, 6.75, 10.0 if k == 2 else 8.0)
        if k == 2:
            st["euler_pre"][12, 1] = -1.25
        # timeout and out of area in the same step: out of area wins (e13); timeout and goal: the goal wins (e14)
        st["progress"][13] = 2999 if k == 5 else 100 + k
        place(st, 13, X0, 7.25, 10.0 if k == 5 else 8.0)
        st["progress"][14] = 3000 if k == 6 else 200 + k
        place(st, 14, X0, 7.75, 0.1 if k == 6 else 8.0)
        seq.append(st)
    return seq


def run(fp32):
    torch.manual_seed(0)
    scene = synth.make_scene(**gg.SCENE_KW)
    digest = gg.scene_digest(scene)
    distn = synth.ray_distribution("37")
    ref = rh.Reference(scene, fp32=fp32, distribution=distn)
    seq = scripted_states(scene)
    eval_res = torch.zeros(E, dtype=torch.long)
    outs = {k: [] for k in ("rock_collision", "reset_buf", "progress_buf", "eval_res", "wheel_min", "body_min")}
    saves = []
    for k, st in enumerate(seq):
        t = ref.make_task(st, curriculum_level=LEVEL[k])
        Rover = t._cls
        t.is_evaluation = True
        t.rover_eval_res = eval_res
        t.global_step = GLOBAL_STEP0 + k
        t._name = NAME
        with tempfile.TemporaryDirectory() as tmp:
            cwd = os.getcwd()
            os.chdir(tmp)
            try:
                with contextlib.redirect_stdout(io.StringIO()):        # the reference's prints
                    t.progress_buf[:] += 1                              # rl_task.py:250
                    Rover.get_observations(t)
                    Rover.calculate_metrics(t)
                    Rover.is_done(t)
                for f in sorted(os.listdir(tmp)):
                    saves.append((k, f, torch.load(os.path.join(tmp, f)).numpy()))
            finally:
                os.chdir(cwd)
        eval_res = t.rover_eval_res.clone()
        wheel, body = ref.rd.get_collisions(t.rover_positions, t.rover_rotation, t._rover.get_joint_positions())
        outs["rock_collision"].append(t.rock_collison.clone())
        outs["reset_buf"].append(t.reset_buf.clone())
        outs["progress_buf"].append(t.progress_buf.clone())
        outs["eval_res"].append(eval_res.clone())
        outs["wheel_min"].append(wheel.float().abs().min(1)[0])
        outs["body_min"].append(body.float().abs().min(1)[0])
    arrays = {"in_" + key: np.stack([st[key].numpy() for st in seq]) for key in seq[0]}
    arrays.update({"out_" + key: np.stack([v.numpy() for v in vs]) for key, vs in outs.items()})
    assert len(saves) == 2 and {s[0] for s in saves} == {T // 2}, [(s[0], s[1]) for s in saves]
    by_name = {s[1]: s[2] for s in saves}
    arrays.update(save_step=np.array(T // 2), save_name_episode_length=np.array(NAME + "episode_length.pt"),
                  save_name_eval_res=np.array(NAME + ".pt"), save_episode_length=by_name[NAME + "episode_length.pt"],
                  save_eval_res=by_name[NAME + ".pt"], curriculum_level=np.array(LEVEL), global_step=GLOBAL_STEP0 + np.arange(T),
                  max_episode_length=np.array(3000), distribution=np.asarray(distn[0], dtype=np.float64),
                  sparse_idx=np.asarray(distn[1], dtype=np.int64), dense_idx=np.asarray(distn[2], dtype=np.int64),
                  scene_digest=np.array(digest), scene_kw=np.array(repr(gg.SCENE_KW)), fp32=np.array(fp32),
                  num_envs_global=np.array(E))
    # a collision decided within 1e-3 of its threshold could differ by a rounding between implementations: the scripted
    # sequence keeps every env clear of that
    thr_w, thr_b = (0.8, 0.45)
    near = (np.abs(arrays["out_wheel_min"] - thr_w) < 1e-3) | (np.abs(arrays["out_body_min"] - thr_b) < 1e-3)
    assert not near.any(), np.argwhere(near)
    return arrays


def main():
    for fp32, name in ((True, "eval_seq_e64_p37_fp32"), (False, "eval_seq_e64_p37_fp16_as_shipped")):
        a = run(fp32)
        codes = a["out_eval_res"][-1]
        print(name, "final codes:", np.bincount(codes, minlength=4), "scripted:", codes[:15].tolist())
        gg.save(name, **a)


if __name__ == "__main__":
    main()
