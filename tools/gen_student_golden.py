"""TEST INFRASTRUCTURE — generates tests/golden/student_small.npz from the reference's own ``Student``
(tasks/utils/learning_by_cheating/student_model.py).

Run in the build container only (needs the reference where oracle/ref_harness.py expects it):

    PYTHONDONTWRITEBYTECODE=1 python tools/gen_student_golden.py

The reference's ``Student.__init__`` loads a teacher checkpoint that does not exist here, so the object is created without it: the
module is allocated, ``nn.Module.__init__`` run, and ``Encoder`` x 2, ``Belief_Encoder``, ``Belief_Decoder`` and ``MLP`` — the
reference's own classes — attached under the names its constructor uses.  ``Belief_Decoder`` appends to the cfg lists it is given,
so it gets copies.  ``forward`` then runs on seeded inputs in float32 on the CPU.

Recorded (data only): the info and the cfg as plain arrays / a JSON string, every parameter under its ``state_dict`` name (``p/<name>``),
``x [B=5, T=6, F]``, ``h0 [n_layers, B, H]`` and the three outputs.  A reduced cfg keeps the file small: the encoder output stays 60
and gb / ga end in 120 (``belief_dim`` is hard-coded to 120 in the reference), the rest shrinks.
"""
from __future__ import annotations

import copy
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from oracle import ref_harness as rh  # noqa: E402

INFO = {"reset": 0, "actions": 2, "proprioceptive": 4, "sparse": 17, "dense": 20}
CFG = {
    "encoder": {"activation_function": "leakyrelu", "encoder_features": [24, 60]},
    "belief_encoder": {"hidden_dim": 44, "n_layers": 2, "activation_function": "leakyrelu", "gb_features": [32, 32, 120], "ga_features": [32, 32, 120]},
    "belief_decoder": {"activation_function": "leakyrelu", "gate_features": [32, 48, 64], "decoder_features": [32, 48, 64]},
    "mlp": {"activation_function": "leakyrelu", "network_features": [64, 48, 32]},
}
B, T = 5, 6


def build_student(info, cfg):
    sys.dont_write_bytecode = True
    if rh.REFERENCE_ROOT not in sys.path:
        sys.path.insert(0, rh.REFERENCE_ROOT)
    from omniisaacgymenvs.tasks.utils.learning_by_cheating import student_model as sm
    cfg = copy.deepcopy(cfg)
    m = sm.Student.__new__(sm.Student)
    torch.nn.Module.__init__(m)
    m.n_re, m.n_pr, m.n_sp, m.n_de, m.n_ac = info["reset"], info["proprioceptive"], info["sparse"], info["dense"], info["actions"]
    m.encoder1 = sm.Encoder(info, cfg["encoder"], encoder="sparse")
    m.encoder2 = sm.Encoder(info, cfg["encoder"], encoder="dense")
    m.belief_encoder = sm.Belief_Encoder(info, cfg["belief_encoder"], input_dim=cfg["encoder"]["encoder_features"][-1] * 2)
    m.belief_decoder = sm.Belief_Decoder(info, copy.deepcopy(cfg["belief_decoder"]), cfg["belief_encoder"]["hidden_dim"])
    m.MLP = sm.MLP(info, cfg["mlp"], belief_dim=120)
    return m.eval()


def main():
    torch.manual_seed(20251)
    torch.set_num_threads(1)
    model = build_student(INFO, CFG)
    with torch.no_grad():
        model.MLP.log_std_parameter.uniform_(-0.5, 0.5)          # not read by forward's outputs; a non-trivial value for the round trip
        f = INFO["proprioceptive"] + INFO["sparse"] + INFO["dense"]
        x = torch.rand(B, T, f) * 2 - 1
        h0 = (torch.rand(CFG["belief_encoder"]["n_layers"], B, CFG["belief_encoder"]["hidden_dim"]) * 2 - 1) * 0.5
        actions, estimated, h = model(x, h0)
    out = {"info_keys": np.array(sorted(INFO)), "info_values": np.array([INFO[k] for k in sorted(INFO)], dtype=np.int64),
           "cfg_json": np.array(json.dumps(CFG, sort_keys=True)), "x": x.numpy(), "h0": h0.numpy(), "actions": actions.numpy(),
           "estimated": estimated.numpy(), "h": h.numpy()}
    for k, v in model.state_dict().items():
        out["p/" + k] = v.numpy().astype(np.float32)
    path = os.path.join(ROOT, "tests", "golden", "student_small.npz")
    np.savez_compressed(path, **out)
    print(f"{path}: {os.path.getsize(path)} bytes, {len(model.state_dict())} parameters, actions {tuple(actions.shape)} "
          f"estimated {tuple(estimated.shape)} h {tuple(h.shape)}")


if __name__ == "__main__":
    main()
