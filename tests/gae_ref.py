"""Sequential float64 reference of GAE(lambda) as include/trpo_engine.h defines it (TRPO_ADV_GAE).

One backward loop over the concatenated paths, one rounding per operation in the order written (Python
floats are IEEE doubles and CPython never contracts a*b+c into an FMA):

    end_t   = t + 1 == n or episode_starts[t+1]
    vnext_t = end_t ? (tail_values ? tail_values[t] : 0) : v_{t+1}
    delta_t = (r_t + gamma * vnext_t) - v_t
    A_t     = end_t ? delta_t : delta_t + (gamma*lambda) * A_{t+1}
    R_t     = end_t ? r_t + gamma * vnext_t : r_t + gamma * R_{t+1}

The loop runs on Python lists: the same arithmetic as numpy float64 scalars at a fraction of the time.
"""
import numpy as np


def gae_ref(rewards, values, gamma, lam, episode_starts=None, tail_values=None):
    """-> (A, R, delta), float64 [n].  values / episode_starts / tail_values may be None (V = 0, one path,
    zero bootstrap values)."""
    r = np.asarray(rewards, np.float64).tolist()
    n = len(r)
    v = [0.0] * n if values is None else np.asarray(values, np.float64).tolist()
    st = [0] * n if episode_starts is None else np.asarray(episode_starts).astype(np.uint8).tolist()
    tail = None if tail_values is None else np.asarray(tail_values, np.float64).tolist()
    gamma, lam = float(gamma), float(lam)
    gl = gamma * lam
    A, R, D = [0.0] * n, [0.0] * n, [0.0] * n
    a_next = r_next = 0.0
    for t in range(n - 1, -1, -1):
        end = t + 1 == n or st[t + 1] != 0
        if end:
            vnext = tail[t] if tail is not None else 0.0
        else:
            vnext = v[t + 1]
        rv = r[t] + gamma * vnext
        delta = rv - v[t]
        if end:
            a_next, r_next = delta, rv
        else:
            a_next, r_next = delta + gl * a_next, r[t] + gamma * r_next
        A[t], R[t], D[t] = a_next, r_next, delta
    return np.array(A, np.float64), np.array(R, np.float64), np.array(D, np.float64)
