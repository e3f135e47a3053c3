"""Test helper (not a test module): hold a value the device stored to the standard normal
its Philox stream prescribes (oracle.noise_normals: purpose 2, process noise;
oracle.policy_normals: purpose 3, action samples), sample by sample.

Each check_* recovers the device's normal from a pair of arrays -- the stored value and
its noiseless counterpart -- computes a per-sample tolerance and asserts
|recovered - prescribed| <= tol on every sample; it returns the worst err / tol.  The
tolerance has one term per float operation between the normal and the stored value, each
half an ulp (np.spacing / 2) of that operation's result, plus one term for the hardware
transcendentals (v_log_f32, v_sqrt_f32, v_sin_f32, v_cos_f32) against float64 Box-Muller
on the exact 24-bit uniforms.  That term is what tests/test_gpu_noise.py's PMSM check has
allowed, and held on hardware, since it was written -- 1e-3 + 1e-5 |nz| at std 3 -- in
units of z: HW(z) = 1e-3 / 3 + 1e-5 |z|, scaled by the sample's own std.  There is no
other constant in here.

An intermediate the device never stores is sized from the prescribed normal; `slack` (the
error bound accumulated so far) is added to its magnitude before the ulp is taken, so a
device value on the far side of a binade boundary is still covered.

Used by tests/test_noise_host.py (a simulated device and its mutations: the check is sharp
before it goes near a GPU), tests/test_gpu_noise.py, tests/test_gpu_policy_sampling.py,
the strengthened policy tests and tools/device_normals_report.py."""
import numpy as np

from conftest import bits_equal

HW_ABS, HW_REL = 1e-3 / 3, 1e-5  # test_gpu_noise.py's 1e-3 + 1e-5 |nz| at std 3, in z units


def hw(z):
    """The hardware-transcendental allowance of a standard normal z, in units of z."""
    return HW_ABS + HW_REL * np.abs(z)


def _hulp(x, T, slack=0.0):
    """Half an ulp, in dtype T, of a value of magnitude |x| + slack: the bound of one
    round-to-nearest to T of a result of that size."""
    v = (np.abs(np.asarray(x, np.float64)) + slack).astype(T)
    return 0.5 * np.spacing(v).astype(np.float64)


def _finish(rec, want, tol, what):
    err = np.abs(rec - want)
    ok = err <= tol  # a NaN fails
    ratio = err / tol
    assert ok.all(), (what, "worst err / tol %.3g" % np.nanmax(np.where(ok, 0.0, ratio)),
                      "%d of %d samples" % ((~ok).sum(), ok.size), np.argwhere(~ok)[:5].tolist())
    return float(ratio.max()) if ratio.size else 0.0


def recover(after, base, dt):
    """(after - base) / T(dt) in float64: the increment per unit of the system's own dt."""
    T = after.dtype
    assert base.dtype == T and T in (np.float32, np.float64)
    return (after.astype(np.float64) - base.astype(np.float64)) / np.float64(T.type(dt))


# ------------------------------------------------------------------ HR (lz_systems.h SysHR::step)
def check_hr(m1, m0, sigma, z, dt, what="hr", detail=None):
    """m1 = m0 + (T)nz * dt with nz = (double)sigma * (double)zf (noise_from_normals).
    m1: the device's master [n, 3]; m0: the noiseless master of the same pre-step state;
    sigma [n]: the env's sigma plane at that step; z [n, 3]: the prescribed normals.
    detail (a dict): "z_err" receives the largest |recovered - prescribed| in units of z."""
    T = m1.dtype
    dtT = np.float64(T.type(dt))
    sg = np.asarray(sigma, np.float64)[:, None]
    want = sg * z                                   # the prescribed noise, float64
    rec = recover(m1, m0, dt)
    tol = sg * hw(z)                                # zf: hardware log / sqrt / cos / sin
    if T == np.float64:                             # (double)sigma * (double)zf: exact for a float32
        tol = tol + _hulp(want, np.float64, tol)    # sigma (24 x 24 bits), one rounding for a float64 one
    tol = tol + _hulp(want, T, tol)                 # (T)nz
    tol = tol + _hulp(want * dtT, T, tol * dtT) / dtT   # (T)nz * dt
    tol = tol + _hulp(m1, T) / dtT                  # m0 + (that): the stored value
    tol = tol + np.spacing(np.abs(rec))             # the recovery's own float64 subtraction and division
    if detail is not None and (sg > 0).any():
        pos = (sg > 0)[:, 0]
        detail["z_err"] = max(detail.get("z_err", 0.0), float((np.abs(rec - want)[pos] / sg[pos]).max()))
    return _finish(rec, want, tol, what)


def hr_step_check(orc, pre, fa, act, post, sigma, z, add_filter, what="hr", detail=None):
    """One teacher-forced HR step: pre / post [n, 6] the device's master and slave before and
    after it, fa [n, 2] the filter memory before it.  The oracle's DEV-mode noiseless step of
    `pre` gives m0; the slave must equal the oracle's bit for bit.  Returns the worst err / tol."""
    st = np.ascontiguousarray(pre.copy())
    f = np.ascontiguousarray(fa.copy())
    with np.errstate(all="ignore"):
        orc.hr_step(st, f, act, None, False, add_filter, orc.DEV)
    assert bits_equal(post[:, 3:], st[:, 3:]), (what, "slave")
    return check_hr(post[:, :3], st[:, :3], sigma, z, orc.PARAMS["hr"][8], what, detail)


# ------------------------------------------------------------------ TP / SC (SysTP / SysSC::step)
def euler_f(orc, key, pre, act):
    """The derivative the noise is added to, in the state's dtype and the device's operation
    order (pmsm3_rhs; TP: of the slave, plus the clipped actions * gain in float32)."""
    T = pre.dtype.type
    p = orc.PARAMS[key]
    x, y, w = (pre[:, 3 + j] for j in range(3)) if key == "tp" else (pre[:, j] for j in range(3))
    pa, pb = T(p[0]), T(p[1])
    with np.errstate(all="ignore"):
        f = np.stack([(-x) + y * w, ((-y) - x * w) + pb * w, pa * (y - w)], 1)
        if key == "tp":
            cl, gain = np.float32(p[4]), np.float32(p[2])
            g = np.clip(act.astype(np.float32), -cl, cl) * gain
            f[:, 0] = f[:, 0] + g[:, 0].astype(T)
            f[:, 1] = f[:, 1] + g[:, 1].astype(T)
    assert f.dtype == pre.dtype
    return f


def check_euler(s1, s_ref, s0, f, std, z, dt, what="euler"):
    """s1 = s0 + (f + (T)nz) * dt with nz = std * (double)zf, against the noiseless
    s_ref = s0 + f * dt.  f: the device's derivative (euler_f); that it is the device's is
    asserted: s0 + f * dt must give s_ref bit for bit."""
    T = s1.dtype
    dtT = np.float64(T.type(dt))
    with np.errstate(all="ignore"):
        q0 = f * T.type(dt)
        assert bits_equal(s0 + q0, s_ref), (what, "f is not the derivative of the noiseless step")
    want = std * z                                  # the prescribed noise, float64
    rec = recover(s1, s_ref, dt)
    f64 = f.astype(np.float64)
    tol = std * hw(z)                               # zf: hardware log / sqrt / cos / sin
    tol = tol + _hulp(want, np.float64, tol)        # std * (double)zf, in double
    tol = tol + _hulp(want, T, tol)                 # (T)nz
    tol = tol + _hulp(f64 + want, T, tol)           # f + (T)nz
    tol = tol + _hulp((f64 + want) * dtT, T, tol * dtT) / dtT   # (that) * dt
    tol = tol + _hulp(s1, T) / dtT                  # s0 + (that): the stored value
    tol = tol + _hulp(q0, T) / dtT                  # the noiseless step's own f * dt
    tol = tol + _hulp(s_ref, T) / dtT               # and its s0 + f * dt
    tol = tol + np.spacing(np.abs(rec))             # the recovery's own float64 subtraction and division
    return _finish(rec, want, tol, what)


def euler_step_check(orc, key, pre, act, post, z, what=None):
    """One teacher-forced TP / SC step (key "tp" / "sc"): pre / post the device's state
    planes before and after it.  The oracle's noiseless step of `pre` gives s0 + f * dt; TP's
    master must equal the oracle's bit for bit.  Returns the worst err / tol."""
    st = np.ascontiguousarray(pre.copy())
    with np.errstate(all="ignore"):
        orc.legacy_step(key, st, None if key == "sc" else act, None)
    p = orc.PARAMS[key]
    sl = slice(3, 6) if key == "tp" else slice(0, 3)
    if key == "tp":
        assert bits_equal(post[:, :3], st[:, :3]), (what or key, "master")
    return check_euler(post[:, sl], st[:, sl], pre[:, sl], euler_f(orc, key, pre, act), p[6], z,
                       p[3], what or key)


# ------------------------------------------------------------------ PMSM (SysPMSM::rhs / step)
PMSM_PLANES = 11  # s1 (3), s2 (3), lambda, Adam m, v, Adam step, episode step


def pmsm_step_check(orc, pre, act, post, z, alpha=0.5, what="pmsm"):
    """One teacher-forced PMSM step: pre / post the device's eleven state planes (a list of
    [n] arrays) before and after it.  The slave is s1 = s0 + (float)((double)t + nz) * dt with
    nz = 3.0 * (double)zf and t the slave's float32 derivative with the actions, against the
    noiseless s0 + t * dt of the oracle's DEV mode; the master must equal the oracle's bit
    for bit.  Returns the worst err / tol."""
    n = act.shape[0]
    S = orc.PmsmState(n)
    S.st[:] = np.stack(pre[:6], 1)
    S.lam[:], S.m[:], S.v[:], S.adam_step[:], S.cur_step[:] = pre[6:11]
    with np.errstate(all="ignore"):
        orc.pmsm_step(S, act, None, False, alpha, orc.DEV)
    s1 = np.stack(post[3:6], 1)
    assert bits_equal(np.stack(post[:3], 1), S.st[:, :3]), (what, "master")
    p = orc.PARAMS["pmsm"]
    sg, gm, dt, fmax = (np.float32(p[j]) for j in (0, 1, 2, 3))
    x = [pre[3 + j] for j in range(3)]
    a = np.clip(act.astype(np.float32), np.float32(-1), np.float32(1)) * fmax
    with np.errstate(all="ignore"):
        t = np.stack([(-x[0] + x[1] * x[2]) + a[:, 0], ((-x[1] - x[0] * x[2]) + gm * x[2]) + a[:, 1],
                      sg * (x[1] - x[2])], 1)
        q0 = t * dt
        s0 = np.stack(x, 1)
        assert t.dtype == np.float32 and bits_equal(s0 + q0, S.st[:, 3:]), (what, "t is not the derivative")
    T, dt64 = np.float32, np.float64(dt)
    want = 3.0 * z                                  # the prescribed noise, float64
    rec = recover(s1, S.st[:, 3:], p[2])
    t64 = t.astype(np.float64)
    tol = 3.0 * hw(z)                               # zf: hardware log / sqrt / cos / sin
    tol = tol + _hulp(want, np.float64, tol)        # 3.0 * (double)zf, in double
    tol = tol + _hulp(t64 + want, np.float64, tol)  # (double)t + nz
    tol = tol + _hulp(t64 + want, T, tol)           # (float)(that)
    tol = tol + _hulp((t64 + want) * dt64, T, tol * dt64) / dt64    # (that) * dt
    tol = tol + _hulp(s1, T) / dt64                 # s0 + (that): the stored value
    tol = tol + _hulp(q0, T) / dt64                 # the noiseless step's own t * dt
    tol = tol + _hulp(S.st[:, 3:], T) / dt64        # and its s0 + t * dt
    tol = tol + np.spacing(np.abs(rec))             # the recovery's own float64 subtraction and division
    return _finish(rec, want, tol, what)


# ------------------------------------------------------------------ action samples (lz_policy.hip normal_rsample)
def check_action(act, mean, scale, z, what="action"):
    """act = mean + zf * scale in float32.  act [n, A]: the device's unclipped samples; mean
    [n, A] or [A]: the exactly known mean; scale [A]: exp(log_std) as the kernel reads it;
    z [n, A]: the prescribed normals.  The comparison is in units of z."""
    act = np.asarray(act)
    assert act.dtype == np.float32
    sc = np.asarray(scale, np.float32).astype(np.float64)
    mean = np.broadcast_to(np.asarray(mean, np.float32), act.shape)
    rec = (act.astype(np.float64) - mean.astype(np.float64)) / sc
    tol = hw(z)                                             # zf: hardware log / sqrt / cos / sin
    tol = tol + _hulp(z * sc, np.float32, tol * sc) / sc    # zf * scale
    tol = tol + _hulp(act, np.float32) / sc                 # mean + (that): the stored value
    tol = tol + np.spacing(np.abs(rec))                     # the recovery's own float64 division
    return _finish(rec, z, tol, what)
