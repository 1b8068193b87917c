"""The contract of srlhip_rollout_policy_summary (include/srlhip.h) restated on the [T][N] planes of the corresponding plane call:
sequential Python / numpy float64 loops, one addition at a time in ascending t, every product rounded before it is added.  A test
helper like tests/policy_act_ref.py: nothing here is shared with the library."""
import numpy as np


def summary_from_planes(obs, reward, done):
    """obs float32 [T][N][D], reward float32 [T][N], done uint8 [T][N] (bit 0 counts) -> {"first" [N] int, "ret" [N] float64,
    "length" [N] int32, "obs_sum", "obs_sqsum" [N][D] float64} as the contract words them"""
    T, N, D = obs.shape
    assert reward.shape == (T, N) and done.shape == (T, N)
    first = np.full(N, T, np.int64)
    ret, length = np.zeros(N, np.float64), np.zeros(N, np.int32)
    obs_sum, obs_sqsum = np.zeros((N, D), np.float64), np.zeros((N, D), np.float64)
    for e in range(N):
        for t in range(T):
            if int(done[t, e]) & 1:
                first[e] = t
                break
        r = np.float64(0.0)
        for t in range(int(first[e])):                  # the reporting step is not counted
            r = r + np.float64(reward[t, e])
        ret[e] = r
        length[e] = min(int(first[e]) + 1, T)
        for d in range(D):
            s, q = np.float64(0.0), np.float64(0.0)
            for t in range(int(length[e])):
                x = np.float64(obs[t, e, d])
                xx = x * x                              # rounded, then added
                s = s + x
                q = q + xx
            obs_sum[e, d], obs_sqsum[e, d] = s, q
    return {"first": first, "ret": ret, "length": length, "obs_sum": obs_sum, "obs_sqsum": obs_sqsum}


def bits_equal(a, b):
    """same dtype, same shape, same bytes (a -0.0 is not a +0.0, a NaN equals itself)"""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def moments_from_sums(count, total, sqtotal):
    """RunningMeanStd.update_from_sums' batch statistics: mean = sum / n, var = sqsum / n - mean^2 clamped at 0 (float64)"""
    n = max(float(count), 1.0)
    mean = np.asarray(total, np.float64) / n
    return mean, np.maximum(np.asarray(sqtotal, np.float64) / n - mean * mean, 0.0)
