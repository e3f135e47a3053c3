"""What float32 itself costs per step, independently of the kernels (runs without a GPU):
every kept (env, step) pair of the reference's float64 trajectories (tests/teacher_forced.py)
is rounded to float32 and stepped once with the float32 oracle (HR in mode DEV), and the
result is held to BASELINE.md's per-step bar, |d| / max(|s|, 1) < 1e-5 on every state
component against the reference's float64 next state, plus the observation / reward bars of
tests/teacher_forced.py.  The bound is the project's 1e-5, not derived from the figures
below.  tests/test_gpu_teacher_forced.py holds the kernels to the same bars.

Measured with the oracle (printed by the test; kept pairs of the fixture's):

  system  pairs          state     obs (non-cancelling)  reward
  L4      12,000/12,000  1.21e-07  5.96e-08              1.34e-07
  HR       8,000/8,000   1.65e-07  9.23e-08              1.59e-07   (no termination mismatch,
                                                        case 6's 201 terminations included)
  T1       4,800/4,800   1.11e-06  0                     1.15e-07
  T2       4,676/4,800   7.07e-07  5.96e-08              rtol 1.46e-07
  TP       4,800/4,800   8.91e-07  5.96e-08              rtol 1.29e-07
  SC       2,400/2,400   1.91e-07  0                     1.05e-07

L4's derivative half f(m) - f(s) cancels (9.43e-05 by the plain measure); scaled by the sum
of the absolute values of its terms (teacher_forced.l4_deriv_scale) the float32 oracle's
largest error over the 12,000 pairs is 1.196e-07, recorded as
teacher_forced.L4_DERIV_SCALED_MAX = 1.20e-07.  This test asserts that the recorded value
is the measured one (to three digits); the GPU test allows the kernel twice it.
"""
import numpy as np
import pytest

import teacher_forced as tf


@pytest.mark.parametrize("key", tf.SYSTEMS)
def test_f32_oracle_step_vs_reference_f64(orc, key):
    P = tf.pairs(orc, key)
    got = tf.step_f32_oracle(orc, key, P)
    fig = tf.measure(orc, key, P, got)
    tf.assert_gates(key, fig, deriv_factor=1.005)
    if key == "l4":
        # the recorded bound is what this oracle measures (three significant digits)
        assert abs(fig["deriv_scaled"] - tf.L4_DERIV_SCALED_MAX) <= 0.005 * tf.L4_DERIV_SCALED_MAX, fig
    if key == "hr":
        # mode REF (glibc pow) and DEV (correctly rounded x^2 / x^3) cost the same
        assert np.array_equal(got["term"], P["term"])
