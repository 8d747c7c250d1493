"""Evaluation mode (rover.py:620-641, 670-672) restated in plain numpy: the yardstick the -m gpu evaluation tests compare the
device latch against.  tests/test_eval_host.py pins it to the reference's own outputs (the eval_seq_* fixtures)."""
import numpy as np

EVAL_FIXTURES = ["eval_seq_e64_p37_fp32", "eval_seq_e64_p37_fp16_as_shipped"]
F = np.float32


def target_dist(pos, target):
    """is_done's f32 distance (rover.py:617): sqrt of the sum of the two squared differences."""
    d = (np.asarray(target, F)[..., 0:2] - np.asarray(pos, F)[..., 0:2]).astype(F)
    sq = (d * d).astype(F)
    return np.sqrt((sq[..., 0] + sq[..., 1]).astype(F))


def restate_step(code, step, rock_collision, td, progress, level, max_episode_length=3000):
    """One step's latch: collision (level >= 2), then out of area (td >= 9.5), goal (td <= 0.18), timeout, each only where the code is
    still 0.  ``progress`` is the post-increment progress.  Returns (codes, latch steps)."""
    code = np.asarray(code, np.int64)
    new = code.copy()
    if level >= 2:
        new = np.where(new == 0, np.asarray(rock_collision, np.int64), new)
    new = np.where((new == 0) & (td >= F(9.5)), 1, new)
    new = np.where((new == 0) & (td <= F(0.18)), 2, new)
    new = np.where((new == 0) & (np.asarray(progress) >= max_episode_length), 3, new)
    return new, np.where(new != code, np.asarray(progress, np.int64), np.asarray(step, np.int64))


def restate_sequence(fx):
    """Codes and latch steps [T, E] of an eval_seq fixture, from its own per-step rock_collision, positions, targets and progress;
    and the save step's two files (episode_length [n, 1], eval_res [E])."""
    n_steps, e = fx["out_eval_res"].shape
    code, step = np.zeros(e, np.int64), np.zeros(e, np.int64)
    codes, steps, saves = [], [], {}
    for k in range(n_steps):
        td = target_dist(fx["in_pos"][k], fx["in_target"][k])
        progress = fx["out_progress_buf"][k]
        code, step = restate_step(code, step, fx["out_rock_collision"][k], td, progress, int(fx["curriculum_level"][k]),
                                  int(fx["max_episode_length"]))
        codes.append(code)
        steps.append(step)
        if int(fx["global_step"][k]) % int(fx["max_episode_length"]) == 0:
            saves[k] = (progress[np.nonzero(code == 2)[0]][:, None], code.copy())
    return np.stack(codes), np.stack(steps), saves
