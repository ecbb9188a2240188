"""Space-time certification of timed trajectories among moving obstacles (ops.moving_clearance, ops.traj_certify_moving,
csrc/mpb_certify_moving.hip; definition and proof: DESIGN.md 10) in numbers: the ONLY definition of its status values, the words of a
trajectory's outputs, the witness-obstacle encoding, the measured slack, and the host side of the chord-against-keyframes deviation
(chord_deviation: pure numpy, fp64).  The interval word, the depth / queue limits, the reach buffer and the Lambda inflation are
certify_layout.py's and are not restated here.  model_gen.py emits include/mpb_st_certify_layout.h from it (which include/mpb.h -- it says
what each name means -- and csrc/mpb_certify_moving.hip include); tests/test_st_certify_cpu.py holds the header text to the generator.
No torch here: model_gen imports it on a build host.
"""
import numpy as np

from . import certify_layout as _CL

# status of a trajectory, value = index: certify_layout.STATUS, then what only the callers above the kernel give (a plan that was not
# found is not certified: STRRTConnect.certify)
STATUS = _CL.STATUS + ('NOT_VALID',)

STC_OUT_INTS = 6                       # per trajectory: status, witness row, witness link, witness obstacle, n_evals, depth_max
STC_OUT_FLOATS = 3                     # per trajectory: witness s, witness eta, margin_cert
# the witness obstacle: o >= 0 a moving obstacle (spheres first, then boxes), -1 - f the static field f of the chain, STC_NO_OBSTACLE none
STC_NO_OBSTACLE = -(1 << 20)

# The slack S: the certificate is a theorem under "|eta as the device computes it - eta| <= S".  The static certifier's value is not
# reused: the interpolated centres add roundings.  S is MEASURED: 32 E_st, E_st the largest |eta fp32 restatement - eta fp64
# restatement| over 10^5 uniform (configuration, segment, s) draws of each scene of tests/st_certify_checks.py (the factor 32 is the one
# the RRT goldens and the static certifier use).  E_st = 2.894e-07 (the 12-joint chain; 2-D point 1.202e-07, Panda 1.422e-07), measured
# 2026-10-21 by `python tests/st_certify_checks.py`.
STC_E_MEASURED = 2.894e-07
STC_DEFAULT_SLACK = 32.0 * STC_E_MEASURED

C_DEFINES = ('STC_OUT_INTS', 'STC_OUT_FLOATS')


def chord_deviation(field, n_rows):
    """max over (obstacle o, interval h, keyframe strictly inside interval h) of |c_o(t_key) - chord_{o,h}(t_key)| in fp64, 0.0 when no
    keyframe lies strictly inside a row interval: how far the field's own piecewise-linear motion is from the chords between the rows'
    centres.  Both are piecewise linear in t, so is their difference, and it vanishes at the rows: its maximum over an interval is at a
    keyframe inside it.  The chord's ends are the fp64 centres of field.rows(n_rows) (the packed buffer rounds them once to fp32, half an ulp or
    about 3e-8 m here: that rounding is left to the slack, and the E_st measurement does NOT cover it -- both of its restatements start
    from the fp32 table)."""
    R = int(n_rows)
    if R < 2:
        return 0.0
    t = field.times(R)
    sc, bc = field.rows(R)
    c = np.concatenate([sc, bc], 1)                                     # (R, O, 3)
    worst = 0.0
    for tk in np.asarray(field.t_key, np.float64):
        h = int(np.searchsorted(t, tk, side='right')) - 1               # t[h] <= tk
        if h < 0 or h >= R - 1 or not t[h] < tk < t[h + 1]:
            continue
        s = (tk - t[h]) / (t[h + 1] - t[h])
        ks, kb = field._centres(np.array([tk]))
        true = np.concatenate([ks, kb], 1)[0]
        chord = c[h] + s * (c[h + 1] - c[h])
        worst = max(worst, float(np.linalg.norm(true - chord, axis=-1).max()))
    return worst
