"""The recurrent student without a GPU: the float64 restatement against the reference's recorded outputs, parameter names, exported
symbols, the cell's route rule, the honesty of the error bound, and the constructor's / load_state_dict's errors."""
import json
import os

import numpy as np
import pytest
import torch

import student_ref as sr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INFO_FULL = {"proprioceptive": 4, "sparse": 20, "dense": 30, "actions": 2}      # default cfg (H = 300) over a short obs row: the act() case of the GPU suite


def load_fixture():
    z = np.load(os.path.join(ROOT, "tests", "golden", "student_small.npz"))
    info = dict(zip(z["info_keys"].tolist(), [int(v) for v in z["info_values"]]))
    cfg = json.loads(str(z["cfg_json"]))
    sd = {k[2:]: torch.from_numpy(z[k]) for k in z.files if k.startswith("p/")}
    return z, info, cfg, sd


def worst(name, got, want, err):
    d = (sr.f64(got) - want).abs()
    ratio = float((d / err).max())
    print(f"{name}: max |d| {float(d.max()):.3e}  max bound {float(err.max()):.3e}  worst d / bound {ratio:.4f}")
    return ratio


def test_float64_restatement_reproduces_the_reference():
    z, info, cfg, sd = load_fixture()
    (a, ea), (s, es), (h, eh) = sr.student_forward_b(sd, info, z["x"], z["h0"])
    assert a.shape == z["actions"].shape and s.shape == z["estimated"].shape and h.shape == z["h"].shape
    for name, want, err, got in (("actions", a, ea, z["actions"]), ("estimated", s, es, z["estimated"]), ("h", h, eh, z["h"])):
        assert worst(name, got, want, err) <= 1.0
    # the propagated bound grows with every layer and step (worst case: every rounding aligned); the first step's is the tightest it gets
    (a1, ea1), (s1, es1), _ = sr.student_forward_b(sd, info, z["x"][:, :1], z["h0"])
    assert worst("actions[t=0]", z["actions"][:, :1], a1, ea1) <= 1.0
    assert worst("estimated[t=0]", z["estimated"][:, :1], s1, es1) <= 1.0


def test_state_dict_has_the_reference_names_and_shapes():
    from isaac_rover_amd.learning.student import StudentPolicy, param_shapes
    _, info, cfg, sd = load_fixture()
    pol = StudentPolicy(None, info, cfg, device="cpu")
    mine = pol.state_dict()
    assert list(mine) == list(sd)
    assert {k: tuple(v.shape) for k, v in mine.items()} == {k: tuple(v.shape) for k, v in sd.items()}
    assert {k: tuple(v) for k, v in param_shapes(info, cfg).items()} == {k: tuple(v.shape) for k, v in sd.items()}
    pol.load_state_dict(sd)
    for k, v in pol.state_dict().items():
        assert torch.equal(v, sd[k]), k
    for name in ("encoder1.encoder.0.layer.0.weight", "belief_encoder.gru.weight_ih_l0", "belief_encoder.gb.2.layer.0.bias",
                 "belief_decoder.gate_encoder.3.layer.0.weight", "MLP.network.3.weight", "MLP.log_std_parameter"):
        assert name in mine
    assert pol.init_hidden(7).shape == (cfg["belief_encoder"]["n_layers"], 7, cfg["belief_encoder"]["hidden_dim"]) and not pol.h.any()


def test_default_cfg_is_the_loaders():
    from isaac_rover_amd.learning.student import DEFAULT_CFG, param_shapes
    assert DEFAULT_CFG["encoder"]["encoder_features"] == [80, 60]
    assert DEFAULT_CFG["belief_encoder"] == {"hidden_dim": 300, "n_layers": 2, "activation_function": "leakyrelu", "gb_features": [128, 128, 120],
                                             "ga_features": [128, 128, 120]}
    assert DEFAULT_CFG["belief_decoder"]["gate_features"] == [128, 256, 512] == DEFAULT_CFG["belief_decoder"]["decoder_features"]
    assert DEFAULT_CFG["mlp"]["network_features"] == [256, 160, 128]
    sh = param_shapes({"proprioceptive": 4, "sparse": 634, "dense": 1112, "actions": 2})
    assert sh["belief_encoder.gru.weight_ih_l0"] == (900, 124) and sh["belief_encoder.gru.weight_hh_l1"] == (900, 300)
    assert sh["MLP.network.0.layer.0.weight"] == (256, 124) and sh["belief_decoder.decoder.3.layer.0.weight"] == (1746, 512)
    assert DEFAULT_CFG["belief_decoder"]["gate_features"] == [128, 256, 512]       # param_shapes appends to copies, not to the cfg


def test_symbols_are_exported_and_listed():
    from isaac_rover_amd import _lib
    _lib.build()
    lib = _lib.load()
    for name in ("rover_gru_cell", "rover_gru_cell_route", "rover_gated_sum"):
        assert name in _lib.SYMBOLS and getattr(lib, name) is not None
    for name in ("gru_cell", "gated_sum", "gru_cell_route"):
        assert callable(getattr(_lib.Engine, name))


def test_gru_cell_route_on_both_sides_of_every_switch_point():
    from isaac_rover_amd._lib import Engine
    route = Engine.gru_cell_route
    assert route(0, 124, 300) == "none" and route(0, 0, 1) == "none"
    # ceil(M / 128) * ceil(H / 32) >= 512 -> four waves per workgroup
    assert route(6528, 3, 300) == "gru_cell<1>" and route(6529, 3, 300) == "gru_cell<4>"
    assert route(65408, 1, 32) == "gru_cell<1>" and route(65409, 1, 32) == "gru_cell<4>"
    assert route(65408, 1, 33) == "gru_cell<4>"                       # 33 columns are two tiles
    assert route(512, 124, 300) == "gru_cell<1>" and route(65536, 124, 300) == "gru_cell<4>"
    assert route(1, 0, 1) == "gru_cell<1>" and route(1, 1 << 20, 1) == "gru_cell<1>"
    # refusals: the hidden width's two ends, negative sizes
    assert route(1, 1, 0) is None and route(1, 1, 32 * 65535) == "gru_cell<4>" and route(1, 1, 32 * 65535 + 1) is None
    assert route(-1, 1, 1) is None and route(1, -1, 1) is None and route(0, 1, 0) is None
    for m, k, hd in sr.CELL_CASES:
        assert route(m, k, hd) in ("gru_cell<1>", "gru_cell<4>")
    assert {route(m, k, hd) for m, k, hd in sr.CELL_CASES} == {"gru_cell<1>", "gru_cell<4>"}


def test_f32_torch_lies_inside_the_bound_on_every_gpu_case():
    """The condition that keeps the bound honest.  Prints the worst error / bound ratio per family (EXPERIMENTS.md §16)."""
    top = 0.0
    for m, k, hd in sr.CELL_CASES:
        if m > 4096:                                                 # the route's switch-point cases: the same arithmetic per row; a slice of rows
            m = 257
        d = sr.cell_data(m, k, hd)
        mask = (torch.arange(m) % 3 == 0)
        for msk in (None, mask):
            got = sr.gru_cell(d["x"], d["h"], d["w_ih"], d["w_hh"], d["b_ih"], d["b_hh"], msk)
            z = lambda t: torch.zeros_like(sr.f64(t))
            want, err = sr.gru_cell_b(sr.f64(d["x"]), z(d["x"]), sr.f64(d["h"]), z(d["h"]), *[sr.f64(d[n]) for n in ("w_ih", "w_hh", "b_ih", "b_hh")], mask=msk)
            top = max(top, float(((sr.f64(got) - want).abs() / err).max()))
    print(f"gru_cell, f32 torch vs float64: worst d / bound {top:.4f}")
    assert top <= 1.0
    top = 0.0
    for m, n in sr.GATED_CASES:
        g = torch.Generator().manual_seed(m * 131 + n)
        add, mul, pre = (torch.rand(m, n, generator=g) * 2 - 1 for _ in range(3))
        pre = pre * 8
        pre.view(-1)[0], pre.view(-1)[-1] = 100.0, -100.0
        z = torch.zeros(m, n, dtype=torch.float64)
        want, err = sr.gated_sum_b(sr.f64(add), z, sr.f64(mul), z, sr.f64(pre), z)
        top = max(top, float(((sr.f64(sr.gated_sum(add, mul, pre)) - want).abs() / err).max()))
    print(f"gated_sum, f32 torch vs float64: worst d / bound {top:.4f}")
    assert top <= 1.0
    # the student: the fixture's sequence, and 12 steps of the default cfg at E = 33 with resets (the GPU suite's act() case)
    zf, info, cfg, sd = load_fixture()
    h, acts, ests = list(torch.from_numpy(zf["h0"])), [], []
    for t in range(zf["x"].shape[1]):
        a, s, h = sr.student_step_f32(sd, info, torch.from_numpy(zf["x"][:, t]), h)
        acts.append(a); ests.append(s)
    (a, ea), (s, es), (hh, eh) = sr.student_forward_b(sd, info, zf["x"], zf["h0"])
    top = max(worst("fixture actions", torch.stack(acts, 1), a, ea), worst("fixture estimated", torch.stack(ests, 1), s, es),
              worst("fixture h", torch.stack(h), hh, eh))
    assert top <= 1.0
    from isaac_rover_amd.learning.student import param_shapes
    sd = sr.random_state_dict(param_shapes(INFO_FULL), seed=3)
    sd64 = {k: sr.f64(v) for k, v in sd.items()}
    obs_seq, resets = act_case_inputs()
    h32 = [torch.zeros(33, 300) for _ in range(2)]
    h64, e64 = [torch.zeros(33, 300, dtype=torch.float64) for _ in range(2)], [torch.zeros(33, 300, dtype=torch.float64) for _ in range(2)]
    top = step_top = 0.0
    for t in range(12):
        a32, _, h32n = sr.student_step_f32(sd, INFO_FULL, obs_seq[t], h32, resets[t])
        a64, ea, _, _, h64, e64 = sr.student_step_b(sd64, INFO_FULL, sr.f64(obs_seq[t]), h64, e64, resets[t])
        top = max(top, float(((sr.f64(a32) - a64).abs() / ea).max()), float(((sr.f64(h32n[1]) - h64[1]).abs() / e64[1]).max()))
        # one step from the f32 state itself (exact inputs): the bound that does not grow with t
        z0 = [torch.zeros(33, 300, dtype=torch.float64) for _ in range(2)]
        a1, ea1, _, _, h1, eh1 = sr.student_step_b(sd64, INFO_FULL, sr.f64(obs_seq[t]), [sr.f64(v) for v in h32], z0, resets[t])
        step_top = max(step_top, float(((sr.f64(a32) - a1).abs() / ea1).max()), float(((sr.f64(h32n[1]) - h1[1]).abs() / eh1[1]).max()))
        h32 = h32n
    print(f"act() x 12, f32 torch vs float64: worst d / propagated bound {top:.3e}; worst d / one-step bound {step_top:.4f}")
    assert top <= 1.0 and step_top <= 1.0


def test_yardstick_check_rejects_wrong_students():
    """The check the GPU suite makes on actions and estimated (student_ref.inside_yardstick) passes the f32 student and fails each of
    student_ref.MUTATIONS — on the fixture's sequence against the recorded f32 outputs, and on one default-cfg step."""
    zf, info, cfg, sd = load_fixture()
    (a, _), (s, _), _ = sr.student_forward_b(sd, info, zf["x"], zf["h0"])

    def fixture_run(mutate):
        h, acts, ests = list(torch.from_numpy(zf["h0"])), [], []
        for t in range(zf["x"].shape[1]):
            av, sv, h = sr.student_step_f32(sd, info, torch.from_numpy(zf["x"][:, t]), h, mutate=mutate)
            acts.append(av); ests.append(sv.expand(zf["x"].shape[0], -1))
        return torch.stack(acts, 1), torch.stack(ests, 1)

    def verdict(acts, ests, a, s, ya, ys):
        (oka, da, ga), (oks, ds, gs) = sr.inside_yardstick(acts, a, ya), sr.inside_yardstick(ests, s, ys)
        return oka and oks, f"actions d {da:.2e} gap {ga:.2e}; estimated d {ds:.2e} gap {gs:.2e}"

    ok, msg = verdict(*fixture_run(None), a, s, zf["actions"], zf["estimated"])
    print("fixture, f32 torch:", msg)
    assert ok, msg
    for m in sr.MUTATIONS:
        ok, msg = verdict(*fixture_run(m), a, s, zf["actions"], zf["estimated"])
        print(f"fixture, {m}:", msg)
        assert not ok, m
    from isaac_rover_amd.learning.student import param_shapes
    sd = sr.random_state_dict(param_shapes(INFO_FULL), seed=3)
    sd64 = {k: sr.f64(v) for k, v in sd.items()}
    obs = act_case_inputs()[0][0]
    g = torch.Generator().manual_seed(4)
    h = [(torch.rand(33, 300, generator=g) * 2 - 1) * 0.5 for _ in range(2)]
    z0 = [torch.zeros(33, 300, dtype=torch.float64) for _ in range(2)]
    a64, _, s64, _, _, _ = sr.student_step_b(sd64, INFO_FULL, sr.f64(obs), [sr.f64(v) for v in h], z0)
    ya, ys, _ = sr.student_step_f32(sd, INFO_FULL, obs, h)
    for m in sr.MUTATIONS:
        am, sm, _ = sr.student_step_f32(sd, INFO_FULL, obs, h, mutate=m)
        ok, msg = verdict(am, sm.expand(33, -1), a64, s64, ya, ys)
        print(f"default cfg, {m}:", msg)
        assert not ok, m


def act_case_inputs():
    """12 observations [33, F] of INFO_FULL and the reset masks of the act() case (rows 3 k at step 4, rows 5 k + 1 at step 9)."""
    g = torch.Generator().manual_seed(99)
    f = INFO_FULL["proprioceptive"] + INFO_FULL["sparse"] + INFO_FULL["dense"]
    obs = [torch.rand(33, f, generator=g) * 2 - 1 for _ in range(12)]
    resets = [None] * 12
    resets[4] = (torch.arange(33) % 3 == 0)
    resets[9] = (torch.arange(33) % 5 == 1)
    return obs, resets


def test_constructor_and_load_errors_name_the_key():
    from isaac_rover_amd.learning.student import DEFAULT_CFG, StudentPolicy
    _, info, cfg, sd = load_fixture()
    with pytest.raises(KeyError, match="dense"):
        StudentPolicy(None, {k: v for k, v in info.items() if k != "dense"}, cfg, device="cpu")
    with pytest.raises(KeyError, match="belief_encoder"):
        StudentPolicy(None, info, {k: v for k, v in cfg.items() if k != "belief_encoder"}, device="cpu")
    bad = json.loads(json.dumps(cfg))
    bad["belief_encoder"]["ga_features"][-1] = 64
    with pytest.raises(ValueError, match="ga_features"):
        StudentPolicy(None, info, bad, device="cpu")
    pol = StudentPolicy(None, info, cfg, device="cpu")
    missing = {k: v for k, v in sd.items() if k != "belief_encoder.gru.bias_hh_l1"}
    with pytest.raises(KeyError, match="belief_encoder.gru.bias_hh_l1"):
        pol.load_state_dict(missing)
    wrong = dict(sd)
    wrong["MLP.network.3.weight"] = torch.zeros(3, 32)
    with pytest.raises(ValueError, match="MLP.network.3.weight"):
        pol.load_state_dict(wrong)
    assert DEFAULT_CFG["belief_encoder"]["hidden_dim"] == 300
