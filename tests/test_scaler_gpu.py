"""GPU: rover_scaler_apply bit for bit against the float32 restatement (tests/scaler_ref.py) and rover_scaler_update against the float64
one under its derived bound (capped at 1e-9 of var + mean^2), at the shapes the plan makes interesting: on both sides of the route
switch and of one chunk, several chunks and a remainder; strided and misaligned x, in place, repetition, two calls in sequence,
skip_if, and a train call plus forward captured in a graph."""
import numpy as np
import pytest
import torch

import scaler_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.fixture(scope="module")
def eng():
    from isaac_rover_amd import _lib
    e = _lib.Engine(64, device=0)
    yield e
    e.close()


def on_gpu(data, stride=None, offset=0):
    """``data`` [m, n] float32 (numpy) on the GPU as a view of rows ``stride`` floats apart, ``offset`` floats into its buffer."""
    m, n = data.shape
    stride = n if stride is None else stride
    buf = torch.full((max(m, 1) * stride + offset,), 77.0, device=DEV)
    view = buf[offset:offset + m * stride].view(m, stride)[:, :n]
    view.copy_(torch.from_numpy(data).to(DEV))
    return view


def bits(t):
    return t.contiguous().view(torch.int32) if t.dtype == torch.float32 else t.contiguous().view(torch.int64)


def same(got, want):
    """``got`` (GPU float32) has the bits of ``want`` (numpy float32); a NaN matches a NaN whatever its payload."""
    g, w = got.cpu().numpy(), np.asarray(want)
    nan = np.isnan(w)
    return g.shape == w.shape and np.array_equal(np.isnan(g), nan) and np.array_equal(g.view(np.int32)[~nan], w.view(np.int32)[~nan])


def dev_state(state):
    mean, var, count = state
    return (torch.from_numpy(np.asarray(mean, dtype=np.float64)).to(DEV), torch.from_numpy(np.asarray(var, dtype=np.float64)).to(DEV),
            torch.tensor([count], dtype=torch.float64, device=DEV))


def scratch_for(m, n):
    from isaac_rover_amd import _lib
    return torch.empty(_lib.scaler_plan(m, n)["scratch_bytes"], dtype=torch.uint8, device=DEV)


# ---- apply -----------------------------------------------------------------------------------------------------------------------------
def apply_case(m, n, seed):
    """Statistics and inputs that reach every branch: +-clip exactly and one ulp beyond after the division, +-Inf, NaN, a zero-variance
    column (the sqrt + eps order decides between 1 / eps and Inf), large and tiny variances."""
    g = np.random.default_rng(seed)
    f = np.float32
    mean = g.normal(size=n) * 3.0
    var = np.exp(g.normal(size=n) * 2.0)
    var[0] = 0.0                                                                   # (x - m) / (0 + eps): huge, clamps; x == m gives 0
    mean[0] = 0.5
    if n > 2:
        var[2], mean[2] = 1.0, 0.0                                                 # scale = 1 + 1e-8 = 1 in f32: y = x, so +-clip is hit exactly
    x = (g.normal(size=(m, n)) * np.sqrt(var) * 3.0 + mean).astype(f)
    if m:
        x[:, 0] = np.where(g.random(m) < 0.5, f(0.5), x[:, 0] + f(1e-6))
    special = [f(5.0), f(-5.0), np.nextafter(f(5.0), f(np.inf)), np.nextafter(f(-5.0), f(-np.inf)), np.nextafter(f(5.0), f(0)), f(np.inf), f(-np.inf),
               f(np.nan), f(0.0), f(-0.0)]
    flat = x.reshape(-1)
    for i, v in enumerate(special):                                               # down column 2 where there is one (y = x there), else wherever
        if n > 2 and i < m:
            x[i, 2] = v
        elif flat.size:
            flat[(i * 7) % flat.size] = v
    return x, mean, var


APPLY_N = [1, 3, 4, 5, 1750]
APPLY_M = [0, 1, 63, 64, 65, 257]


@pytest.mark.parametrize("n", APPLY_N)
@pytest.mark.parametrize("m", APPLY_M)
def test_apply_bit_for_bit(eng, m, n):
    x, mean, var = apply_case(m, n, seed=1000 * n + m)
    dmean, dvar, _ = dev_state((mean, var, 1.0))
    for inverse in (False, True):
        want = R.inverse(x, mean, var) if inverse else R.forward(x, mean, var)
        forms = {"contiguous": on_gpu(x), "stride n + 3": on_gpu(x, n + 3), "off 16-byte alignment": on_gpu(x, n + (n % 2), offset=1),
                 "even stride, 8-byte base": on_gpu(x, n + 2 + (n % 2), offset=2)}
        for label, xv in forms.items():
            got = eng.scaler_apply(xv, dmean, dvar, inverse=inverse)
            assert got.shape == (m, n)
            assert same(got, want), (label, inverse, m, n)
            out = on_gpu(np.zeros_like(x), n + 5, offset=3)                        # strided, misaligned out
            eng.scaler_apply(xv, dmean, dvar, out, inverse=inverse)
            assert same(out, want), (label, "strided out", inverse, m, n)
            eng.scaler_apply(xv, dmean, dvar, xv, inverse=inverse)                 # in place
            assert same(xv, want), (label, "in place", inverse, m, n)
    if m >= 10 and n > 2:                                                          # every special sits in column 2: they did what the definition says
        y = R.forward(x, mean, var)
        assert list(y[:7, 2]) == [5.0, -5.0, 5.0, -5.0, float(np.nextafter(np.float32(5.0), np.float32(0))), 5.0, -5.0] and np.isnan(y[7, 2])
        assert np.all(np.isin(y[:, 0], (0.0, 5.0, -5.0)) | np.isnan(y[:, 0]))      # zero variance: (x - m) / eps clamps unless x == m


def test_apply_in_place_leaves_the_padding_alone(eng):
    x, mean, var = apply_case(65, 5, seed=9)
    dmean, dvar, _ = dev_state((mean, var, 1.0))
    whole = torch.full((65 * 8 + 1,), 77.0, device=DEV)
    view = whole[1:].view(65, 8)[:, :5]
    view.copy_(torch.from_numpy(x).to(DEV))
    eng.scaler_apply(view, dmean, dvar, view)
    assert bool((whole[1:].view(65, 8)[:, 5:] == 77.0).all()) and float(whole[0]) == 77.0


def test_apply_python_layer(eng):
    from isaac_rover_amd._lib import RoverError
    mean, var = torch.zeros(4, dtype=torch.float64, device=DEV), torch.ones(4, dtype=torch.float64, device=DEV)
    x = torch.zeros(8, 4, device=DEV)
    for bad in (dict(x=x.double()), dict(x=x.cpu()), dict(mean=mean.float()), dict(var=var[:3]), dict(out=torch.zeros(8, 5, device=DEV))):
        kw = dict(x=x, mean=mean, var=var, out=None)
        kw.update(bad)
        with pytest.raises(RoverError):
            eng.scaler_apply(kw["x"], kw["mean"], kw["var"], kw["out"])
    big = torch.zeros(200, device=DEV)
    with pytest.raises(RoverError, match="without being the same array"):          # one refusal of the C layer through a live ctx
        eng.scaler_apply(big[:32].view(8, 4), mean, var, big[4:36].view(8, 4))
    assert eng.scaler_apply(torch.empty(0, 4, device=DEV), mean, var).shape == (0, 4)


# ---- update ----------------------------------------------------------------------------------------------------------------------------
def update_data(m, n, seed):
    """Magnitudes <= 8; column 0 a constant with a large mean (cancellation), column 1 (where there is one) +-8 alternating."""
    g = np.random.default_rng(seed)
    x = g.uniform(-8.0, 8.0, size=(m, n)).astype(np.float32)
    x[:, 0] = 7.75
    if n > 1:
        x[:, 1] = np.where(np.arange(m) % 2 == 0, 8.0, -8.0)
    if n > 3:
        x[:, 3] = (x[:, 3] * 0.01 + 6.0).astype(np.float32)                       # small spread on a large mean
    return x


def check_state(got, state, x, n_chunks, label):
    """The device's state against the restatement's from ``state`` on ``x``, under the derived bound capped at CAP (var + mean^2)."""
    want = R.update(state, x)
    d_mean, d_var = R.update_bound(state, x, n_chunks)
    # the restatement's own two-halves error stays inside the cap for these inputs: checked here, on the CPU
    h = x.shape[0] // 2
    if h >= 2 and x.shape[0] - h >= 2:
        mb, vb = R.batch_moments(x)
        (ma, va), (mc, vc) = R.batch_moments(x[:h]), R.batch_moments(x[h:])
        na, nc = float(h), float(x.shape[0] - h)
        m2 = va * (na - 1) + vc * (nc - 1) + (mc - ma) ** 2 * na * nc / (na + nc)
        assert np.all(np.abs(m2 / (na + nc - 1) - vb) <= R.CAP * (vb + mb ** 2)), f"{label}: the inputs are too hard for the cap"
    b_mean, b_var = R.capped(d_mean, d_var, want[0], want[1])
    gm, gv, gc = (t.cpu().numpy() for t in got)
    assert gc[0] == want[2], f"{label}: count {gc[0]} != {want[2]}"
    e_mean, e_var = np.abs(gm - want[0]), np.abs(gv - want[1])
    tiny = np.finfo(np.float64).tiny
    print(f"{label}: worst mean error / bound {float((e_mean / np.maximum(b_mean, tiny)).max()):.3f}, var {float((e_var / np.maximum(b_var, tiny)).max()):.3f}; "
          f"derived bound / cap at most {float((d_var / (R.CAP * (want[1] + want[0] ** 2))).max()):.2e}")
    assert np.all(e_mean <= b_mean), f"{label}: mean off by up to {e_mean.max()} (bound {b_mean[e_mean.argmax()]})"
    assert np.all(e_var <= b_var), f"{label}: var off by up to {e_var.max()} (bound {b_var[e_var.argmax()]})"
    return want


def update_shapes():
    """(m, n) from the plan: N one below, at and one above the route switch; M = 2; M one below, at and one above one chunk; three chunks
    and a remainder; N = 1 with M = 4 097; N = 1750 with M = 130."""
    from isaac_rover_amd import _lib
    switch = max(n for n in range(1, 64) if _lib.scaler_plan(100, n)["route"] == _lib.SCALER_NARROW)
    shapes = [(2, 1), (4097, 1), (130, 1750), (2, 1750)]
    for n in (switch - 1, switch, switch + 1):
        rows = _lib.scaler_plan(100, n)["rows_per_chunk"]
        shapes += [(2, n), (rows - 1, n), (rows, n), (rows + 1, n), (3 * rows + 5, n)]
    big = _lib.scaler_plan(10 ** 6, switch + 1)["rows_per_chunk"]                  # the wide route's larger chunk, past its switch in M
    shapes += [(8192, switch + 1), (8193, switch + 1), (8192 + 3 * big + 7, 11)]
    return shapes


def test_update_shapes_cover_the_plan():
    from isaac_rover_amd import _lib
    shapes = update_shapes()
    routes = {_lib.scaler_plan(m, n)["route"] for m, n in shapes}
    chunks = {_lib.scaler_plan(m, n)["n_chunks"] for m, n in shapes}
    sizes = {_lib.scaler_plan(m, n)["rows_per_chunk"] for m, n in shapes}
    assert routes == {_lib.SCALER_WIDE, _lib.SCALER_NARROW} and {1, 2, 4} <= chunks and len(sizes) == 3


@pytest.mark.parametrize("m,n", update_shapes())
def test_update_against_the_restatement(eng, m, n):
    from isaac_rover_amd import _lib
    x = update_data(m, n, seed=m * 31 + n)
    plan = _lib.scaler_plan(m, n)
    state = R.fresh(n)
    dstate = dev_state(state)
    xv = on_gpu(x)
    scratch = scratch_for(m, n)
    eng.scaler_update(xv, *dstate, scratch)
    check_state(dstate, state, x, plan["n_chunks"], f"[{m}, {n}] fresh")
    assert float(dstate[1][0]) == (1.0 + 7.75 ** 2 * m / (m + 1)) / (m + 1)        # the constant column: M2 exactly 0, every sum exact in f64
    # the same call repeated on a fresh state: the same bits; strided and offset x: the same bits as contiguous
    for label, other in (("repeat", xv), ("odd stride", on_gpu(x, n + 3)), ("4 bytes off", on_gpu(x, n + (n % 2), offset=1)),
                         ("even stride", on_gpu(x, n + 2 + (n % 2), offset=2))):
        again = dev_state(state)
        eng.scaler_update(other, *again, scratch)
        for a, b in zip(again, dstate):
            assert torch.equal(bits(a), bits(b)), (label, m, n)
    # a second call in sequence, against the restatement from ITS first result
    y = update_data(max(m // 2, 2), n, seed=m + n + 1) * np.float32(0.5) + np.float32(1.0)
    host1 = tuple(t.cpu().numpy() if i < 2 else float(t.cpu()[0]) for i, t in enumerate(dstate))
    eng.scaler_update(on_gpu(y), *dstate, scratch_for(y.shape[0], n))
    check_state(dstate, host1, y, _lib.scaler_plan(y.shape[0], n)["n_chunks"], f"[{m}, {n}] second call")


def test_update_skip_if_and_refusals(eng):
    from isaac_rover_amd._lib import RoverError
    x = on_gpu(update_data(300, 12, seed=4))
    state = dev_state(R.update(R.fresh(12), update_data(50, 12, seed=5)))
    before = [t.clone() for t in state]
    flag = torch.ones(1, dtype=torch.int32, device=DEV)
    scratch = scratch_for(300, 12)
    eng.scaler_update(x, *state, scratch, skip_if=flag)
    for a, b in zip(state, before):
        assert torch.equal(bits(a), bits(b))                                      # nonzero: bit-unchanged
    flag.zero_()
    eng.scaler_update(x, *state, scratch, skip_if=flag)
    plain = [t.clone() for t in before]
    eng.scaler_update(x, *plain, scratch)
    for a, b, c in zip(state, plain, before):
        assert torch.equal(bits(a), bits(b)) and not torch.equal(bits(a), bits(c))  # zero: the same bits as without a flag
    with pytest.raises(RoverError, match="at least 2"):
        eng.scaler_update(x[:1], *state, scratch)
    with pytest.raises(RoverError, match="plan needs"):
        eng.scaler_update(x, *state, scratch[:-1])
    with pytest.raises(RoverError):
        eng.scaler_update(x, *state, scratch, skip_if=torch.ones(1, dtype=torch.int64, device=DEV))


# ---- RunningStandardScaler -------------------------------------------------------------------------------------------------------------
def test_scaler_object_shapes_and_train_then_forward(eng):
    from isaac_rover_amd.learning.preprocess import RunningStandardScaler
    g = np.random.default_rng(8)
    x3 = (g.normal(size=(4, 16, 6)) * 2 + 1).astype(np.float32)
    s = RunningStandardScaler(eng, 6)
    y = s(torch.from_numpy(x3).to(DEV), train=True)                               # updates first, normalises with the new statistics
    want = R.update(R.fresh(6), x3)
    check_state((s.running_mean, s.running_variance, s.current_count), R.fresh(6), x3.reshape(-1, 6), 1, "object [T, E, size]")
    assert y.shape == (4, 16, 6)
    now = (s.running_mean.cpu().numpy(), s.running_variance.cpu().numpy())
    assert same(y, R.forward(x3, *now))
    assert not np.array_equal(R.forward(x3, *now), R.forward(x3, *R.fresh(6)[:2])) and want[2] == 65.0
    # size 1: [M], [T, E], [M, 1] and [T, E, 1] are the same rows
    v = (g.normal(size=(4, 16)) * 30 + 100).astype(np.float32)
    outs = []
    for shape in ((64,), (4, 16), (64, 1), (4, 16, 1)):
        s1 = RunningStandardScaler(eng, 1)
        t = torch.from_numpy(v.reshape(shape)).to(DEV)
        o = s1(t, train=True)
        assert o.shape == shape
        outs.append((bits(o).reshape(-1).cpu(), bits(s1.running_mean).cpu(), bits(s1.running_variance).cpu()))
        back = s1(o, inverse=True)
        assert back.shape == shape and float((back - t).abs().max()) <= 1e-3 * 130
        t2 = t.clone()
        assert s1(t2, out=t2).data_ptr() == t2.data_ptr() and torch.equal(bits(t2).reshape(-1).cpu(), bits(s1(t)).reshape(-1).cpu())      # in place
    for o in outs[1:]:
        assert all(torch.equal(a, b) for a, b in zip(o, outs[0]))
    with pytest.raises(ValueError, match="at least 2"):
        RunningStandardScaler(eng, 6)(torch.zeros(1, 6, device=DEV), train=True)
    with pytest.raises(ValueError):
        RunningStandardScaler(eng, 6)(torch.zeros(4, 5, device=DEV))
    with pytest.raises(ValueError, match="skip_if"):
        RunningStandardScaler(eng, 6)(torch.zeros(4, 6, device=DEV), skip_if=torch.zeros(1, dtype=torch.int32, device=DEV))
    # state_dict round trip on the device
    s2 = RunningStandardScaler(eng, 6)
    s2.load_state_dict({k: t.cpu() for k, t in s.state_dict().items()})
    xq = torch.from_numpy(x3).to(DEV)
    assert torch.equal(bits(s2(xq)), bits(s(xq)))


def test_train_then_forward_captured_in_a_graph(eng):
    from isaac_rover_amd.learning.preprocess import RunningStandardScaler
    g = np.random.default_rng(12)
    batches = [torch.from_numpy((g.normal(size=(257, 41)) * (i + 1) + i).astype(np.float32)).to(DEV) for i in range(3)]
    eager = RunningStandardScaler(eng, 41)
    eager_out = [eager(b, train=True).clone() for b in batches]
    s = RunningStandardScaler(eng, 41)
    static_in, static_out = batches[0].clone(), torch.empty(257, 41, device=DEV)
    s(static_in, train=True, out=static_out)                                      # warm-up: the scratch has its size
    s.load_state_dict(RunningStandardScaler(None, 41, device="cpu").state_dict())  # back to the initial state, in place
    torch.cuda.synchronize()
    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(stream):
        with torch.cuda.graph(graph, stream=stream):
            s(static_in, train=True, out=static_out)
    torch.cuda.current_stream().wait_stream(stream)
    s.load_state_dict(RunningStandardScaler(None, 41, device="cpu").state_dict())  # (a capture runs nothing, but be explicit)
    for b, want in zip(batches, eager_out):
        static_in.copy_(b)
        graph.replay()
        assert torch.equal(bits(static_out), bits(want))
    torch.cuda.synchronize()
    for a, b in zip((s.running_mean, s.running_variance, s.current_count), (eager.running_mean, eager.running_variance, eager.current_count)):
        assert torch.equal(bits(a), bits(b))
    assert float(s.current_count) == 1 + 3 * 257
