"""The bf16 student's entry points, routes, reference data and bounds on the CPU (tests/gru_bf16_ref.py); the GPU side is
tests/test_student_bf16_gpu.py."""
import pytest
import torch

import gru_bf16_ref as G
import student_ref as sr
from bf16_ref import rd

NEW_SYMBOLS = ("rover_gru_cell_bf16", "rover_gru_cell_route_bf16", "rover_linear_forward_bf16", "rover_linear_route_bf16")


def test_symbols_are_exported_and_listed():
    from isaac_rover_amd import _lib
    _lib.build()
    lib = _lib.load()
    for name in NEW_SYMBOLS:
        assert name in _lib.SYMBOLS and getattr(lib, name) is not None


def test_routes_name_one_instantiation_and_refuse_what_f32_refuses():
    from isaac_rover_amd._lib import Engine
    cell = lambda m, k, h: Engine.gru_cell_route(m, k, h, precision="bf16")
    assert cell(0, 124, 300) == "none" and cell(0, 0, 1) == "none"
    names = {cell(m, k, h) for m, k, h in G.LATTICE_CASES + sr.CELL_CASES + [(512, 424, 300), (65536, 424, 300), (1, 1 << 20, 1)]}
    assert names == {"gru_cell_bf16<128,64>"}                        # one instantiation at every batch size
    for m, k, h in ((1, 1, 0), (1, 1, 32 * 65535 + 1), (-1, 1, 1), (1, -1, 1), (0, 1, 0), (0, -1, 3)):
        assert cell(m, k, h) is None and Engine.gru_cell_route(m, k, h) is None      # the f32 cell's refusals, no more and no fewer
    assert cell(1, 1, 32 * 65535) == "gru_cell_bf16<128,64>"
    lin = lambda m, k, n: Engine.linear_route(m, k, n, precision="bf16")
    assert lin(0, 3, 7) == "none"
    assert {lin(m, k, n) for m in (1, 17, 129, 65536) for k in (0, 1, 300) for n in (1, 120, 256)} == {"linear_bf16<128,128>"}
    for m, k, n in ((1, 1, 257), (1, 1, 0), (-1, 1, 1), (1, -1, 1), (0, 1, 257)):
        assert lin(m, k, n) is None and Engine.linear_route(m, k, n) is None
    with pytest.raises(ValueError):
        Engine.gru_cell_route(1, 1, 1, precision="fp16")
    with pytest.raises(ValueError):
        Engine.linear_route(1, 1, 1, precision="fp16")


@pytest.fixture(scope="module")
def lattice_cases():
    """Every lattice cell of the GPU suite, built once (the builder asserts exactness and the presence of non-representable operands)."""
    return {(m, k, h, fam): G.lattice_cell(m, k, h, fam) for m, k, h in G.LATTICE_CASES for fam in G.FAMILIES}


def test_lattice_builder_covers_the_lists_and_keeps_its_promises(lattice_cases):
    ms, ks, hs = ({c[i] for c in G.LATTICE_CASES} for i in range(3))
    assert ms == {1, 15, 16, 17, 31, 32, 33, 127, 128, 129, 257} and ks == {0, 1, 31, 32, 33, 124, 300}
    assert hs == {1, 15, 16, 17, 31, 32, 33, 44, 300, 63, 64, 65}
    assert (129, 124, 300) in G.LATTICE_CASES and (33, 300, 300) in G.LATTICE_CASES and len(G.LATTICE_CASES) == 25
    for (m, k, h, fam), (d, counts) in lattice_cases.items():
        assert float(d["x"].abs().max()) <= (2.0 if fam == "a" else 1.0) if k else True
        assert float(d["h"].abs().max()) <= 1.0 and float(d["b_ih"].abs().max()) <= 0.5
        # the four pre-activations of the rounded operands are the same in f32 as in float64: sums in two orders, then the biases
        xr, hr, wi, wh = (rd(sr.f64(d[n])) for n in ("x", "h", "w_ih", "w_hh"))
        want = xr @ wi.T + hr @ wh.T + sr.f64(d["b_ih"]) + sr.f64(d["b_hh"])
        for flip in (False, True):
            f = (lambda t: t.flip(1)) if flip else (lambda t: t)
            got = ((f(xr.float()) @ f(wi.float()).T + f(hr.float()) @ f(wh.float()).T) + d["b_ih"]) + d["b_hh"]
            assert torch.equal(got.double(), want), (m, k, h, fam, flip)


def test_f32_emulation_in_two_orders_lies_inside_the_lattice_bound(lattice_cases):
    top = 0.0
    for (m, k, h, fam), (d, _) in lattice_cases.items():
        mask = (torch.arange(m) % 3 == 1) if m > 2 else None
        want, err = G.cell_bound(d, mask, exact_sums=True)
        fwd, rev = G.emulate_cell(d, mask), G.emulate_cell(d, mask, reverse=True)
        assert torch.equal(fwd, rev), (m, k, h, fam)                 # exact sums: the order cannot matter
        ratio = float(((fwd.double() - want).abs() / err).max())
        top = max(top, ratio)
        assert ratio <= 1.0, (m, k, h, fam, ratio)
        assert float(err.max()) < 4e-6                               # what remains of the bound: the epilogue alone
    print(f"lattice cells, f32 emulation: worst error / bound {top:.3f}")


def test_lattice_bound_rejects_the_four_mutants(lattice_cases):
    checked = 0
    for (m, k, h, fam), (d, counts) in lattice_cases.items():
        if sum(counts) < 100:                                        # (1, 0, 1), (15, 1, 15) and the like: too few elements to count on
            continue
        want, err = G.cell_bound(d, exact_sums=True)
        for mutant in G.MUTANTS:
            bad = int(((G.emulate_cell(d, mutant=mutant).double() - want).abs() > err).sum())
            assert bad > 0, (m, k, h, fam, mutant)
        checked += 1
    assert checked >= 40                                             # nearly every case of the list is large enough to count


def test_cell_bound_is_gru_cell_b_where_the_two_coincide():
    """cell_bound restates student_ref.gru_cell_b: with operands that ARE representable (so that rounding and the choice of h in the
    blend change nothing) the two give the same value and the same bound."""
    d = {n: rd(sr.f64(v)).float() for n, v in sr.cell_data(33, 124, 44).items()}
    z = lambda t: torch.zeros_like(sr.f64(t))
    mask = torch.arange(33) % 4 == 1
    want, err = sr.gru_cell_b(sr.f64(d["x"]), z(d["x"]), sr.f64(d["h"]), z(d["h"]), *[sr.f64(d[n]) for n in ("w_ih", "w_hh", "b_ih", "b_hh")], mask=mask)
    got, gerr = G.cell_bound(d, mask)
    assert torch.equal(got, want) and torch.allclose(gerr, err, rtol=1e-12, atol=0)


def test_real_valued_emulation_lies_inside_the_rounded_operand_bound():
    top = 0.0
    for m, k, h in [c for c in sr.CELL_CASES if c[0] <= 65]:
        d = sr.cell_data(m, k, h)
        want, err = G.cell_bound(d)
        for rev in (False, True):
            top = max(top, float(((G.emulate_cell(d, reverse=rev).double() - want).abs() / err).max()))
    print(f"real-valued cells, f32 emulation: worst error / bound {top:.3f}")
    assert top <= 1.0


def test_student_policy_rejects_unknown_precisions():
    from isaac_rover_amd.learning.student import StudentPolicy
    from test_student_host import INFO_FULL
    for bad in ("fp16", "BF16", None, 16):
        with pytest.raises(ValueError, match="precision"):
            StudentPolicy(None, INFO_FULL, device="cpu", precision=bad)
    pol = StudentPolicy(None, INFO_FULL, device="cpu", precision="bf16")
    assert pol.precision == "bf16" and StudentPolicy(None, INFO_FULL, device="cpu").precision == "f32"
    assert all(v.dtype == torch.float32 for v in pol.state_dict().values())          # no bf16 copy of the weights
    obs = torch.zeros(3, 54)
    with pytest.raises(ValueError, match="precision"):
        pol.act(obs, precision="fp16")
    with pytest.raises(ValueError, match="precision"):
        pol.forward(obs[None], torch.zeros(2, 1, 300), precision="half")
