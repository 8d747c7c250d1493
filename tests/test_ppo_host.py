"""CPU: the closed-form PPO gradients of tests/ppo_ref.py against float64 autograd of the loss expressions, the training symbols and
the backward route query of the library (host only), and PPO's argument checks."""
import ctypes as C
import types

import pytest
import torch

import ppo_ref as P


@pytest.mark.parametrize("variant", ["reference", "entropy", "no_value_clip", "no_log_std_clip"])
@pytest.mark.parametrize("A,log_std", [(1, [0.3]), (2, [-0.4, 2.5]), (3, [-21.0, 0.1, -0.7])])
def test_closed_form_gradients_match_autograd(A, log_std, variant):
    cfg = dict(P.PPO_CFG)
    cfg.update({"entropy": {"entropy_loss_scale": 0.01, "value_loss_scale": 0.5}, "no_value_clip": {"clip_predicted_values": False},
                "no_log_std_clip": {"clip_log_std": False}}.get(variant, {}))
    if variant == "no_log_std_clip":
        log_std = [min(max(v, -3.0), 2.5) for v in log_std]
    d = P.ppo_data(120, A, seed=3 + A, device="cpu", log_std=log_std, cfg=cfg)
    want, _, fragile = P.ppo_loss(d, cfg)
    assert not bool(fragile.any())
    D = {k: v.double() for k, v in d.items()}
    # every branch is present: r inside / below / above, both signs of advantage (and zero), value - old inside / outside
    z = (D["actions"] - D["mean"]) / torch.exp(P._ls_clamped(d["log_std"], cfg))
    r = torch.exp(((-0.5 * z * z - P._ls_clamped(d["log_std"], cfg)) - P.HALF_LOG_2PI).sum(1) - D["old_log_prob"])
    for rsel in (r < 0.8, (r >= 0.8) & (r <= 1.2), r > 1.2):
        for asel in (D["advantages"] > 0, D["advantages"] < 0):
            assert bool((rsel & asel).any())
    dv = (D["value"] - D["old_values"]).abs()
    assert bool((dv < 0.2).any()) and bool((dv > 0.2).any()) and bool((D["advantages"] == 0).any())
    mean, ls, value = (D[k].clone().requires_grad_(True) for k in ("mean", "log_std", "value"))
    pol, val, ent, kl = P.ppo_loss_expr(mean, ls, value, D, cfg)
    (pol + val + ent).backward()
    for name, got, ref in (("d_mean", want["d_mean"], mean.grad), ("d_value", want["d_value"], value.grad), ("d_log_std", want["d_log_std"], ls.grad),
                           ("stats", want["stats"], torch.stack((pol, val, ent, kl)).detach())):
        scale = float(ref.abs().max())
        assert torch.allclose(got, ref, rtol=1e-12, atol=1e-12 * scale), (name, float((got - ref).abs().max()), scale)
    if A > 1 and cfg["clip_log_std"]:
        assert float(want["d_log_std"][1 if A == 2 else 0]) == 0.0          # a log_std outside its clamp gets no gradient


def test_library_exports_training_symbols_and_routes():
    from isaac_rover_amd import _lib
    lib = C.CDLL(_lib.LIB_PATH)
    for name in ("rover_linear_backward", "rover_ppo_loss", "rover_linear_backward_route"):
        assert hasattr(lib, name), name
        assert name in _lib.SYMBOLS
    R = _lib.Engine.linear_backward_route
    assert R(5, 3, 257, False) is None and R(5, 257, 3, True) is None
    assert R(5, 257, 3, False) == "wgrad<1,1>/1" and R(0, 3, 3, True) == "zero" and R(-1, 3, 3, False) is None
    assert R(512, 1112, 80, False) == "wgrad<1,1>/8" and R(65536, 1112, 80, False) == "wgrad<3,4>/64"
    assert R(65536, 124, 256, True) == "wgrad<3,4>/64;dgrad<4,4>" and R(5, 0, 3, True) == "wgrad<1,1>/1"


def test_ppo_rejects_bad_cfg():
    from isaac_rover_amd.learning.ppo import DEFAULT_CONFIG, PPO
    assert DEFAULT_CONFIG == {"learning_epochs": 4, "mini_batches": 60, "discount_factor": 0.99, "lambda": 0.95, "learning_rate": 1e-4,
                              "grad_norm_clip": 1.0, "ratio_clip": 0.2, "value_clip": 0.2, "clip_predicted_values": True,
                              "entropy_loss_scale": 0.0, "value_loss_scale": 1.0, "kl_threshold": 0.008}
    mem = types.SimpleNamespace(memory_size=4, num_envs=8)
    with pytest.raises(ValueError, match="unknown cfg keys"):
        PPO(None, None, None, mem, {"learning_rate": 1e-3, "learning_rates": 1e-3})
    for mb in (0, 33):
        with pytest.raises(ValueError, match="mini_batches"):
            PPO(None, None, None, mem, {"mini_batches": mb})
