"""GPU: the simulation smoother (dsge_simulation_smoother_batched, csrc/dsge_simsmooth.hpp) against its numpy restatement
(tests/simulation_smoother_reference.py: simulate x+, form y*, oracle.kalman_filter_logp, rts_smoother, add x+ / eps+ back) on the
read-only edge cases of tests/smoother_cases.py (2-3 draws, 8 steps, one missing entry: the smallest shapes that reach every LDS
class), with the draws from a per-case seeded numpy generator.

Bar: the project's fixed 1e-9 x scale per block -- states: max(1, max|x~_ref|), shocks: max sqrt(Q_jj) (cases.scales)."""
import functools

import numpy as np
import pytest
from numpy.testing import assert_array_equal

import oracle
from geconpy_amd import _frontend as F
from geconpy_amd import _lib, batched

from tests import smoother_cases as cases
from tests.simulation_smoother_reference import simulation_smoother

pytestmark = pytest.mark.gpu

BAR = 1e-9
MAX_PATHS = 33


@functools.lru_cache(maxsize=None)
def _draws(name, with_d=False):
    """(x0 (nb, S, m), eps (nb, S, n, k), eta (nb, S, n, p), d) for S = MAX_PATHS paths per draw: model-sized, read-only; a call
    with fewer paths takes the first ones."""
    c = cases.case(name)
    nb, m, k = c["R"].shape
    n, p = c["y"].shape
    rng = np.random.default_rng([29, *name.encode()])
    sd = np.stack([np.sqrt(np.diag(cases.q_full(c, i))) for i in range(nb)])
    H = np.broadcast_to(c["H"], (nb, p))
    x0 = 0.02 * rng.standard_normal((nb, MAX_PATHS, m))
    eps = rng.standard_normal((nb, MAX_PATHS, n, k)) * sd[:, None, None, :]
    eta = rng.standard_normal((nb, MAX_PATHS, n, p)) * np.sqrt(H)[:, None, None, :]
    d = rng.normal(0, 0.01, p) if with_d else c["d"]
    for a in (x0, eps, eta, d):
        if a is not None:
            a.setflags(write=False)
    return x0, eps, eta, d


def _panel(c, complete):
    """The case's panel; ``complete``: its missing entry replaced by 0 (without the F jitter a missing entry leaves a zero on the
    diagonal of F, and the REFERENCE itself stops with a singular matrix: tests/smoother_cases.py::forward_fail has none either)."""
    return np.nan_to_num(c["y"], nan=0.0) if complete else c["y"]


@functools.lru_cache(maxsize=None)
def _reference(name, n_paths, conv=None, with_d=False, complete=False):
    """{draw: (x~ (S, n, m), eps~ (S, n, k))} for the draws of the case that have a reference (computed once, shared)."""
    c = cases.case(name)
    x0, eps, eta, d = _draws(name, with_d)
    conv = c["conv"] if conv is None else dict(conv)
    cv = None if conv is None else oracle.FilterConventions(**conv)
    out = {}
    for i in c["draws"]:
        x = cases.draw(c, i)
        di = d if with_d else x["d"]
        res = [simulation_smoother(_panel(c, complete), x["T"], x["R"], x["Q"], x["Z"], x["H"], di, x0[i, s], eps[i, s], eta[i, s], conventions=cv)
               for s in range(n_paths)]
        out[i] = (np.stack([r[0] for r in res]), np.stack([r[1] for r in res]))
    return out


def _run(name, n_paths, with_d=False, sl=slice(None), zero=False, complete=False, **kw):
    """The device on the draws ``sl`` of the case with the first ``n_paths`` paths of its draws."""
    c = cases.case(name)
    x0, eps, eta, d = _draws(name, with_d)
    own = lambda x, shared_ndim: x if x is None or x.ndim == shared_ndim else x[sl]  # noqa: E731
    q = c["q"][sl] if c["q_mode"].endswith("batched") else c["q"]
    if zero:  # (eta = None would make the front end draw one: Hdiag is given)
        dr = dict(x0=np.zeros_like(x0[sl, :n_paths]), eps=np.zeros_like(eps[sl, :n_paths]), eta=np.zeros_like(eta[sl, :n_paths]))
    else:
        dr = dict(x0=x0[sl, :n_paths], eps=eps[sl, :n_paths], eta=eta[sl, :n_paths])
    dr.update(kw)
    return batched.simulation_smoother_batched(c["T"][sl], c["R"][sl], q, own(c["Z"], 2), _panel(c, complete), n_paths=n_paths, d=own(d, 1),
                                               Hdiag=own(c["H"], 1), q_mode=c["q_mode"], **dr)


def _check(name, out, ref, draws=None):
    c = cases.case(name)
    for i, (xr, er) in ref.items():
        if draws is not None and i not in draws:
            continue
        sc, ec = max(1.0, np.abs(xr).max()), np.sqrt(np.diag(cases.q_full(c, i))).max()
        assert np.isnan(out["shocks"][i, :, 0]).all() and np.isnan(er[:, 0]).all()
        errs = (np.abs(out["states"][i] - xr).max() / sc, np.abs(out["shocks"][i, :, 1:] - er[:, 1:]).max() / ec if er.shape[1] > 1 else 0.0)
        print(name, "draw", i, "paths", xr.shape[0], "errors / scale (states, shocks):", errs)
        assert errs[0] <= BAR and errs[1] <= BAR, (name, i, errs)


@pytest.mark.parametrize("name", cases.PARITY_CASES)
def test_parity(name):
    """Three paths per draw against the reference on every parity case: m = 1, 2, 16, 32, 33, 48, 49, 64; r = m; k = m = 64; p = 1
    and 16; full, singular and per-draw Q; per-draw Z, d, Hdiag; T_len = 2 and 3."""
    out = _run(name, 3)
    assert (out["status"] == 0).all()
    _check(name, out, _reference(name, 3))
    c = cases.case(name)
    if c.get("zero_shock") is not None:  # eps+ = 0 in a shock without variance: its draw stays exactly 0
        eps = np.array(_draws(name)[1][:, :3])
        eps[..., c["zero_shock"]] = 0.0
        out0 = _run(name, 3, eps=eps)
        assert (out0["shocks"][:, :, 1:, c["zero_shock"]] == 0.0).all()


@pytest.mark.parametrize("name", ["zc16", "zc33", "zc49", "dense64_p16"])
@pytest.mark.parametrize("n_paths", [1, 16, 17, 33])
def test_group_edges(name, n_paths):
    """One path, a full group, a group and one path, two groups and one path, against the reference."""
    out = _run(name, n_paths)
    assert (out["status"] == 0).all()
    ref = {i: (x[:n_paths], e[:n_paths]) for i, (x, e) in _reference(name, MAX_PATHS).items()}
    _check(name, out, ref)


@pytest.mark.parametrize("name", ["zc16", "zc33", "zc49", "dense64_p16"])
def test_a_path_does_not_depend_on_its_group(name):
    """Each path of the 17-path call is bit-identical to a one-path call with that path's draws."""
    x0, eps, eta, _ = _draws(name)
    out = _run(name, 17)
    for s in range(17):
        one = _run(name, 1, x0=x0[:, s:s + 1], eps=eps[:, s:s + 1], eta=eta[:, s:s + 1])
        for key in ("states", "shocks"):
            assert_array_equal(out[key][:, s], one[key][:, 0], err_msg=f"{key}, path {s}")
        assert_array_equal(out["ll"], one["ll"])


@pytest.mark.parametrize("name", ["zc16", "zc49", "dense33_qfull", "obs_batched"])
def test_zero_draws_equal_the_smoother(name):
    """x0 = 0, eps = 0, eta = NULL: the smoothed means of kalman_smoother_batched at 1e-9 x scale, its ll bit for bit.  The
    numpy wrapper draws an eta when it gets None next to an Hdiag, so eta = NULL (and x0 = NULL) go through the C entry itself,
    and the wrapper's call with zero arrays must equal that one bit for bit."""
    c = cases.case(name)
    out = _run(name, 2, zero=True)
    nb, m, k = c["R"].shape
    n, p = c["y"].shape
    b = F.HOST
    raw = dict(states=np.empty((nb, 2, n, m)), shocks=np.empty((nb, 2, n, k)), ll=np.empty((nb, n)), status=np.zeros(nb, dtype=np.int32))
    Q = b.inp(c["q"])
    F.call(b, "dsge_simulation_smoother_batched", T=b.inp(c["T"]), R=b.inp(c["R"]), Q=Q, q_mode=F.q_layout(Q.shape, c["q_mode"], nb, k),
           **F.obs_args(b, c["Z"], c["d"], c["H"], nb, p, m), y=b.inp(c["y"]), batch=nb, m=m, k=k, p=p, T_len=n, jitter=batched.JITTER_DEFAULT,
           missing_fill=batched.MISSING_FILL, rank_tol=0.0, scratch_limit_bytes=0, x0=None, x0_batched=0, eps=np.zeros((2, n, k)),
           eps_batched=0, eta=None, eta_batched=0, n_paths=2, ll_out=raw["ll"], x_out=raw["states"], eps_out=raw["shocks"],
           status_io=raw["status"])
    for key in raw:
        assert_array_equal(out[key], raw[key], err_msg=key)
    sm = batched.kalman_smoother_batched(c["T"], c["R"], c["q"], c["Z"], c["y"], d=c["d"], Hdiag=c["H"], q_mode=c["q_mode"])
    assert (out["status"] == 0).all() and (sm["status"] == 0).all()
    assert_array_equal(out["ll"], sm["ll"])
    for i in range(c["T"].shape[0]):
        sc, ec = max(1.0, np.abs(sm["smoothed_states"][i]).max()), np.sqrt(np.diag(cases.q_full(c, i))).max()
        for s in range(2):
            errs = (np.abs(out["states"][i, s] - sm["smoothed_states"][i]).max() / sc,
                    np.abs(out["shocks"][i, s, 1:] - sm["smoothed_shocks"][i, 1:]).max() / ec)
            print(name, i, s, "zero draws - smoother / scale:", errs)
            assert max(errs) <= BAR, errs


def test_draw_array_forms():
    """Shared ([n_paths] ...) against the same arrays broadcast per draw, for x0, eps, eta: bit-identical; eta = None with Hdiag."""
    name = "zc33"
    x0, eps, eta, _ = _draws(name)
    nb = x0.shape[0]
    sh = dict(x0=x0[0, :5], eps=eps[0, :5], eta=eta[0, :5])
    ref = _run(name, 5, **{key: np.ascontiguousarray(np.broadcast_to(v, (nb, *v.shape))) for key, v in sh.items()})
    for key in sh:
        mixed = {k2: (v if k2 == key else np.ascontiguousarray(np.broadcast_to(v, (nb, *v.shape)))) for k2, v in sh.items()}
        out = _run(name, 5, **mixed)
        for o in ("states", "shocks", "ll", "status"):
            assert_array_equal(out[o], ref[o], err_msg=f"{key} shared: {o}")
    out = _run(name, 5, eta=None)
    assert (out["status"] == 0).all() and np.isfinite(out["states"]).all()
    assert np.abs(out["states"] - _run(name, 5)["states"]).max() > 0


@pytest.mark.parametrize("conv,with_d", [(dict(jitter_on_F=False), False), (dict(mask_d=True), True), (dict(mask_d=False), True),
                                         (dict(joseph=False), False)])
def test_conventions(conv, with_d):
    """sw17_qfull under the other filter conventions (mask_d on and off with a non-zero d), against the reference under the same
    FilterConventions.  Without the F jitter the panel is taken complete (``_panel``): with the case's missing entry the reference
    has no value to compare with."""
    name = "sw17_qfull"
    complete = conv.get("jitter_on_F") is False
    out = _run(name, 3, with_d=with_d, complete=complete, options=_lib.filter_conventions(**conv))
    assert (out["status"] == 0).all()
    _check(name, out, _reference(name, 3, tuple(sorted(conv.items())), with_d, complete))


def _own(name, i, n_paths, **kw):
    return _run(name, n_paths, sl=slice(i, i + 1), **kw)


def test_incoming_status_gives_nan_in_every_path():
    name = "obs_batched"
    status = np.array([0, _lib.ST_NOT_CONVERGED, 0], dtype=np.int32)
    out = _run(name, 17, status=status)
    assert out["status"].tolist() == [0, _lib.ST_NOT_CONVERGED, 0]
    assert np.isnan(out["states"][1]).all() and np.isnan(out["shocks"][1]).all() and np.isnan(out["ll"][1]).all()
    _check(name, out, {i: (x[:17], e[:17]) for i, (x, e) in _reference(name, 17).items()}, draws=(0, 2))
    for i in (0, 2):
        own = _own(name, i, 17)
        for key in ("states", "shocks", "ll"):
            assert_array_equal(out[key][i], own[key][0], err_msg=f"{key}, draw {i}")


def test_forward_failure_gives_nan_in_every_path():
    name = "forward_fail"
    opts = _lib.filter_conventions(**cases.case(name)["conv"])
    out = _run(name, 17, options=opts)
    assert out["status"][1] & _lib.ST_FILTER_NONFINITE and out["status"][0] == 0 and out["status"][2] == 0
    assert np.isnan(out["states"][1]).all() and np.isnan(out["shocks"][1]).all()
    _check(name, out, _reference(name, 17))
    for i in (0, 2):
        own = _own(name, i, 17, options=opts)
        for key in ("states", "shocks", "ll"):
            assert_array_equal(out[key][i], own[key][0], err_msg=f"{key}, draw {i}")


def test_singular_m_keeps_the_last_step():
    name = "singular_m_nojit"
    c = cases.case(name)
    opts = _lib.filter_conventions(**c["conv"])
    out = _run(name, 17, options=opts)
    assert out["status"].tolist() == [0, _lib.ST_SMOOTHER_SINGULAR, 0]
    assert np.isfinite(out["states"][1, :, -1]).all() and np.isfinite(out["ll"][1]).all()
    assert np.isnan(out["states"][1, :, :-1]).all() and np.isnan(out["shocks"][1]).all()
    x0, eps, eta, _ = _draws(name)
    filt = batched.kalman_filter_outputs_batched(c["T"], c["R"], c["q"], c["Z"], c["y"], Hdiag=c["H"], q_mode=c["q_mode"], options=opts)
    assert_array_equal(out["ll"], filt["ll"])
    _check(name, out, _reference(name, 17))
    for i in (0, 2):
        own = _own(name, i, 17, options=opts)
        for key in ("states", "shocks", "ll"):
            assert_array_equal(out[key][i], own[key][0], err_msg=f"{key}, draw {i}")


def test_chunked_equals_unchunked():
    """scratch_limit_bytes of one draw's figure (three chunks of one draw) against the default: bit-identical."""
    name = "obs_batched"
    c = cases.case(name)
    m, n = c["T"].shape[1], c["y"].shape[0]
    one = _run(name, 17)
    chunked = _run(name, 17, scratch_limit_bytes=batched.simulation_smoother_scratch_bytes_per_draw(m, n, 17))
    tiny = _run(name, 17, scratch_limit_bytes=1)
    assert (one["status"] == 0).all()
    for key in ("states", "shocks", "ll", "status"):
        assert_array_equal(one[key], chunked[key], err_msg=key)
        assert_array_equal(one[key], tiny[key], err_msg=key)


def test_engine_equals_host_twin():
    """LogpEngine.simulation_smoother on device tensors, on a non-default torch stream: bit-identical to the host twin."""
    import torch
    from geconpy_amd.engine import LogpEngine

    name = "obs_batched"
    c = cases.case(name)
    x0, eps, eta, _ = _draws(name)
    ref = _run(name, 17)
    eng = LogpEngine(0)
    dev = {x: eng.to_device(np.array(c[x])) for x in ("T", "R", "q", "Z", "y", "H", "d")}
    dr = {key: eng.to_device(np.ascontiguousarray(v[:, :17])) for key, v in (("x0", x0), ("eps", eps), ("eta", eta))}
    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(stream):
        out = eng.simulation_smoother(dev["T"], dev["R"], dev["q"], dev["Z"], dev["y"], n_paths=17, d=dev["d"], Hdiag=dev["H"],
                                      q_mode=c["q_mode"], **dr)
    stream.synchronize()
    for key in ("states", "shocks", "ll", "status"):
        assert_array_equal(out[key].cpu().numpy(), ref[key], err_msg=key)


@pytest.mark.parametrize("name", ["zc33", "dense33"])
def test_stationary_factor(name):
    """F F' = P0 at 1e-12 x max|P0|, host and engine."""
    import torch
    from geconpy_amd.engine import LogpEngine

    c = cases.case(name)
    P0, _, st = batched.lyapunov_batched(c["T"], c["R"], c["q"], q_mode=c["q_mode"])
    assert (st == 0).all()
    F = batched.stationary_factor(c["T"], c["R"], c["q"], q_mode=c["q_mode"])
    eng = LogpEngine(0)
    Fd = eng.stationary_factor(*(eng.to_device(np.array(c[x])) for x in ("T", "R", "q")), q_mode=c["q_mode"])
    torch.cuda.synchronize()
    for tag, f in (("host", F), ("engine", Fd.cpu().numpy())):
        err = np.abs(f @ np.swapaxes(f, 1, 2) - P0).max() / np.abs(P0).max()
        print(name, tag, "|F F' - P0| / max|P0|:", err)
        assert err <= 1e-12, (tag, err)


def test_generated_draws():
    """rng=7, return_draws=True is reproduced bit for bit by a second call given the returned x0, eps, eta; two seeds give
    different paths; a full (singular) Q and the engine's generator make draws of the right shapes."""
    import torch
    from geconpy_amd.engine import LogpEngine

    name = "zc33"
    c = cases.case(name)
    args = (c["T"], c["R"], c["q"], c["Z"], c["y"])
    kw = dict(n_paths=3, Hdiag=c["H"], q_mode=c["q_mode"])
    a = batched.simulation_smoother_batched(*args, rng=7, return_draws=True, **kw)
    assert (a["status"] == 0).all() and np.isfinite(a["states"]).all()
    assert a["x0"].shape == (2, 3, 33) and a["eps"].shape == (2, 3, 8, 5) and a["eta"].shape == (2, 3, 8, 4)
    b = batched.simulation_smoother_batched(*args, x0=a["x0"], eps=a["eps"], eta=a["eta"], **kw)
    for key in ("states", "shocks", "ll"):
        assert_array_equal(a[key], b[key], err_msg=key)
    other = batched.simulation_smoother_batched(*args, rng=8, **kw)
    assert np.abs(other["states"] - a["states"]).max() > 1e-6
    c2 = cases.case("dense33_qfull_zero")
    f = batched.simulation_smoother_batched(c2["T"], c2["R"], c2["q"], c2["Z"], c2["y"], n_paths=2, Hdiag=c2["H"], q_mode=c2["q_mode"],
                                            rng=1, return_draws=True)
    assert (f["status"] == 0).all() and f["eps"].shape == (2, 2, 8, 5) and np.isfinite(f["states"]).all()
    Qe = np.einsum("bstj,bstl->bjl", f["eps"], f["eps"])  # (the factor of a singular Q stays in its range, up to the eigensolver)
    assert np.abs(Qe[:, c2["zero_shock"], c2["zero_shock"]]).max() <= 1e-12 * np.abs(Qe).max()
    eng = LogpEngine(0)
    gen = torch.Generator(device=eng.device)
    gen.manual_seed(7)
    dev = [eng.to_device(np.array(c[x])) for x in ("T", "R", "q", "Z", "y")]
    g = eng.simulation_smoother(*dev, n_paths=3, Hdiag=eng.to_device(np.array(c["H"])), q_mode=c["q_mode"], generator=gen,
                                return_draws=True)
    torch.cuda.synchronize()
    h = batched.simulation_smoother_batched(*args, x0=g["x0"].cpu().numpy(), eps=g["eps"].cpu().numpy(), eta=g["eta"].cpu().numpy(), **kw)
    for key in ("states", "shocks", "ll"):
        assert_array_equal(g[key].cpu().numpy(), h[key], err_msg=key)
