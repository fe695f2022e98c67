"""Numpy reference of the Kalman likelihood across dated structural breaks (TEST INFRASTRUCTURE ONLY; a helper, not a test module):
one draw, ``oracle.kalman_filter_logp`` chained segment by segment with the boundary step of docs/design/segmented_filter.md.

Period t belongs to segment s(t) = max{s : seg_start[s] <= t}; the matrices of segment s drive the transition INTO every period of s
and the observation OF every period of s.  Between the last period of s and the first of s' = s + 1:
    a = T_s' (a_filt + shift_s');   P = sym(T_s' P_filt T_s'') + sym(R_s' Q_s' R_s'')
"""
import numpy as np

import oracle


def _sym(A):
    return 0.5 * (A + A.T)


def segment_of(seg_start, t):
    return int(np.searchsorted(np.asarray(seg_start), t, side="right") - 1)


def segmented_filter(y, segs, seg_start, a0=None, P0=None, shift=None, jitter=oracle.JITTER_DEFAULT,
                     missing_fill_value=oracle.MISSING_FILL, conventions=None):
    """``segs``: one dict(T, R, Q (k, k), Z, H (p, p) or None, d (p,) or None) per segment; ``shift``: (S, m) or None (row 0 is
    never read).  Returns dict(logp, ll (n,), a_last, P_last: the filtered moments of the last period, P_pred (n, m, m))."""
    y = np.atleast_2d(np.asarray(y, dtype=np.float64))
    n, S = y.shape[0], len(segs)
    bounds = list(seg_start) + [n]
    a, P = a0, P0
    ll, p_pred = [], []
    for s, x in enumerate(segs):
        if s > 0:  # the boundary step, with the matrices of the segment being entered
            af = a if shift is None else a + np.asarray(shift)[s]
            a = x["T"] @ af
            P = _sym(x["T"] @ P @ x["T"].T) + _sym(x["R"] @ x["Q"] @ x["R"].T)
        _, ll_s, stt = oracle.kalman_filter_logp(y[bounds[s]:bounds[s + 1]], x["T"], x["R"], x["Q"], x["Z"], H=x["H"], d=x["d"], a0=a,
                                                 P0=P, jitter=jitter, missing_fill_value=missing_fill_value, return_states=True,
                                                 conventions=conventions)
        ll.append(ll_s)
        p_pred.append(stt["P_pred"])
        a, P = stt["a_filt"][-1], stt["P_filt"][-1]
    ll = np.concatenate(ll)
    return dict(logp=float(ll.sum()), ll=ll, a_last=a, P_last=P, P_pred=np.concatenate(p_pred))


def innovation_conditions(y, segs, seg_start, res, jitter=oracle.JITTER_DEFAULT, missing_fill_value=oracle.MISSING_FILL,
                          conventions=None):
    """cond_2 of the innovation covariance F_t = Z P_{t|t-1} Z' + H + jit_F I of every period, on its OBSERVED entries (a missing
    entry's row and column of the masked F hold the jitter alone and decide nothing); 1 for a period with nothing observed."""
    cv = oracle.DEFAULT_CONVENTIONS if conventions is None else conventions
    out = []
    for t in range(np.shape(y)[0]):
        x = segs[segment_of(seg_start, t)]
        obs = ~(np.isnan(y[t]) | (y[t] == missing_fill_value))
        if not obs.any():
            out.append(1.0)
            continue
        Z = x["Z"][obs]
        H = np.zeros((len(obs), len(obs))) if x["H"] is None else x["H"]
        F = Z @ res["P_pred"][t] @ Z.T + H[np.ix_(obs, obs)] + (jitter if cv.jitter_on_F else 0.0) * np.eye(int(obs.sum()))
        out.append(float(np.linalg.cond(F)))
    return np.array(out)
