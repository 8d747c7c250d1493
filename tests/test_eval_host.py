"""CPU: evaluation mode's numpy restatement (tests/eval_helpers.py) against the reference's own evaluation branch, and the
multi-GPU summary reduction on gloo."""
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT, load_golden
from eval_helpers import EVAL_FIXTURES, restate_sequence, restate_step, target_dist


@pytest.mark.parametrize("name", EVAL_FIXTURES)
def test_restatement_matches_reference(name):
    fx = load_golden(name)
    codes, steps, saves = restate_sequence(fx)
    np.testing.assert_array_equal(codes, fx["out_eval_res"])
    # the latch step is the progress of the step at which the code first became non-zero
    for e in range(codes.shape[1]):
        nz = np.nonzero(codes[:, e])[0]
        assert steps[-1, e] == (fx["out_progress_buf"][nz[0], e] if len(nz) else 0)
    assert list(saves) == [int(fx["save_step"])]
    ep_len, res = saves[int(fx["save_step"])]
    assert fx["save_episode_length"].shape == ep_len.shape and ep_len.shape[1] == 1
    np.testing.assert_array_equal(fx["save_episode_length"], ep_len)
    np.testing.assert_array_equal(fx["save_eval_res"], res)
    assert str(fx["save_name_eval_res"]) == "rover_eval_no_noise_teacher_rocks_small_area_removedv5.pt"
    assert str(fx["save_name_episode_length"]) == "rover_eval_no_noise_teacher_rocks_small_area_removedv5episode_length.pt"


@pytest.mark.parametrize("name", EVAL_FIXTURES)
def test_fixture_covers_the_cases(name):
    """The scripted envs of tools/gen_eval_golden.py do what the generator says they do."""
    fx = load_golden(name)
    td = np.stack([target_dist(p, t) for p, t in zip(fx["in_pos"], fx["in_target"])])
    r, c, lvl = fx["out_eval_res"], fx["out_rock_collision"], fx["curriculum_level"]
    f = np.float32
    assert td[2, 0] == f(0.18) and r[2, 0] == 2 and r[-1, 0] == 2 and td[-1, 0] >= 9.5       # goal at 0.18, then out of area: stays 2
    assert td[2, 1] == np.nextafter(f(0.18), f(1)) and r[2, 1] == 0 and r[3, 1] == 2
    assert td[1, 2] == f(9.5) and r[1, 2] == 1 and fx["out_reset_buf"][1, 2] == 0           # out of area: code 1, no reset
    assert td[3, 3] == np.nextafter(f(9.5), f(0)) and r[3, 3] == 0 and r[4, 3] == 1
    assert (td[:, 4] > 9.5).all() and (td[:, 4] < 11).all() and (fx["out_reset_buf"][:, 4] == 0).all()
    assert td[2, 5] >= 11 and fx["out_reset_buf"][2, 5] == 1
    assert fx["out_progress_buf"][1, 6] == 3000 and r[0, 6] == 0 and r[1, 6] == 3
    assert fx["out_reset_buf"][1, 7] == 1 and r[6, 7] == 0 and r[7, 7] == 2                   # tilt reset: no code
    assert (c[lvl == 1][:, 9] == 0).all() and r[2, 9] == 0 and c[3, 9] == 1 and r[3, 9] == 1  # level 1: no latch
    assert c[4, 10] == 1 and td[4, 10] <= 0.18 and r[3, 10] == 0 and r[4, 10] == 1            # collision beats goal
    assert r[0, 11] == 2
    assert (np.bincount(r[-1], minlength=4) > 0).all()


def test_restate_step_precedence():
    z = np.zeros(4, np.int64)
    code, step = restate_step(z, z, [1, 0, 0, 0], np.array([0.1, 9.5, 0.1, 5.0], np.float32), np.array([3000, 3000, 3000, 3000]), 2)
    assert code.tolist() == [1, 1, 2, 3] and step.tolist() == [3000] * 4
    code2, step2 = restate_step(code, step, [0, 1, 1, 1], np.array([9.9, 0.1, 9.9, 0.1], np.float32), np.array([7, 7, 7, 7]), 2)
    assert code2.tolist() == code.tolist() and step2.tolist() == step.tolist()                # once set, never changes
    code3, _ = restate_step(z, z, [1, 1, 1, 1], np.array([5.0] * 4, np.float32), np.array([1] * 4), 1)
    assert code3.tolist() == [0] * 4                                                          # level 1: no collision latch


_WORKER = r"""
import os, sys, torch, torch.distributed as dist
sys.path.insert(0, os.environ["ROVER_ROOT"])
from isaac_rover_amd.distributed import reduce_eval_summary
dist.init_process_group("gloo")
rank = dist.get_rank()
shards = [torch.tensor([5, 3, 2, 1, 0, 40, 900, 3000], dtype=torch.int64), torch.tensor([1, 0, 7, 0, 0, 0, 12345, 0], dtype=torch.int64)]
s = shards[rank].clone()
out = reduce_eval_summary(s)
assert out is s and out.dtype == torch.int64
assert torch.equal(out, shards[0] + shards[1]), out
print(f"rank {rank} ok")
"""


def test_reduce_eval_summary_world_size_2_gloo(tmp_path):
    script = tmp_path / "worker.py"
    script.write_text(_WORKER)
    port = 31500 + (os.getpid() % 2000)
    procs = []
    for r in range(2):
        env = dict(os.environ, RANK=str(r), WORLD_SIZE="2", MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), ROVER_ROOT=ROOT)
        procs.append(subprocess.Popen([sys.executable, str(script)], env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True))
    outs = [p.communicate(timeout=120)[0] for p in procs]
    for r, (p, o) in enumerate(zip(procs, outs)):
        assert p.returncode == 0, o
        assert f"rank {r} ok" in o
