"""Path certification by clearance bisection (ops.clearance, ops.path_certify, csrc/mpb_certify.hip; definition and proof: DESIGN.md 10) in
numbers: the ONLY definition of its status values, limits, the packed interval word, the default slack and the reach buffer, and the host
side of the motion bound (reach_table, motion_bound, pack_reach: pure numpy).  model_gen.py emits include/mpb_certify_layout.h from it
(which include/mpb.h -- it says what each name means -- and csrc/mpb_certify.hip include); tests/test_certify_cpu.py holds the header text
to the generator.  No torch here: model_gen imports it on a build host.
"""
import numpy as np

# status of a path, value = index
STATUS = ('FREE', 'COLLISION', 'UNDECIDED_DEPTH', 'UNDECIDED_QUEUE', 'BAD_INPUT', 'BUFFER_CHANGED')

# an interval of the queue is one word: segment << CERT_J_BITS | j, the j-th of the 2^d intervals of its segment at level d
CERT_J_BITS = 20
CERT_MAX_DEPTH = 20                    # j < 2^20 fills the low field; the midpoint parameter (2j + 1) 2^-(d+1) is exact in fp32 up to here
CERT_MAX_ROWS = 1 << (32 - CERT_J_BITS)   # rows of a path: its segments 0 .. rows - 2 fill the high field
CERT_MAX_INTERVALS = 4096              # intervals of one level: two queues of that many words in LDS (32 KB)
CERT_MAX_LINKS = 1024                  # collision spheres of a robot the reach buffer serves
CERT_OUT_INTS = 5                      # per path: status, witness segment, witness link, n_evals, depth_max
CERT_OUT_FLOATS = 3                    # per path: witness t, witness eta, margin_cert
CERT_DEFAULT_MAX_DEPTH = 16            # (the RRT planners leave nodes on the margin surface: what 12 levels leave undecided, 13 .. 15 mostly decide)
CERT_DEFAULT_MAX_INTERVALS = 1024

# The slack S: the certificate is a theorem under "|eta as the device computes it - eta| <= S".  S is MEASURED, not derived: 32 E, E the
# largest |eta fp32 restatement - eta fp64 oracle| over 10^5 uniform configurations of each scene of tests/certify_checks.py (the
# factor 32 is the one the RRT goldens use for E_gap).  E = 2.894e-07 (the 12-joint chain; 2-D point 1.202e-07, Panda 1.422e-07),
# measured 2026-10-21 by `python tests/certify_checks.py`.
CERT_E_MEASURED = 2.894e-07
CERT_DEFAULT_SLACK = 32.0 * CERT_E_MEASURED

# the reach buffer: a header of REACH_HEADER_WORDS words (magic, n_dof, n_links, kind), then rho as [n_dof][n_links] fp32
REACH_MAGIC = 0x4D504252               # 'MPBR'
REACH_HEADER_WORDS = 4
# what the device multiplies its fp32 sum Lambda_l by, so that it is an upper bound of the real sum: 1 + 2^-20 clears the 13 roundings
# (12 fma and the product) of relative 2^-24 each
CERT_LAMBDA_INFLATE_C = '0x1.00001p+0f'
CERT_LAMBDA_INFLATE = 1.0 + 2.0 ** -20

C_DEFINES = ('CERT_J_BITS', 'CERT_MAX_DEPTH', 'CERT_MAX_ROWS', 'CERT_MAX_INTERVALS', 'CERT_MAX_LINKS', 'CERT_OUT_INTS', 'CERT_OUT_FLOATS',
             'REACH_HEADER_WORDS')


def reach_table(rs):
    """rho (n_dof, n_links) fp32 of a robot spec (Robot.spec()): sphere l is never farther than rho[i, l] from the origin of joint i
    when joint i moves it, 0 when it does not.  The chain is frame_{j+1} = frame_j P_j Rz(q_j); sphere l sits on frame f_l at offset
    o_l; joint i turns about the z axis through the point frame_i P_i puts the origin at, and moves sphere l iff i < f_l.  Then
        x_l - origin_i = R (transl(P_{i+1}) + R' (transl(P_{i+2}) + ... + R'' o_l))      (rotations only: norms are kept)
        |x_l - origin_i| <= rho_il = sum_{j=i+1}^{f_l-1} |transl(P_j)| + |o_l|.
    Summed in fp64 and rounded UP to fp32.  A point robot (kind 0) has no joints to bound: its table is all ones and motion_bound
    takes the Euclidean length of the step instead."""
    D, L = int(rs['n_dof']), len(rs['link_radius'])
    if int(rs['kind']) == 0:
        return np.ones((D, L), np.float32)
    tl = np.linalg.norm(np.asarray(rs['joint_tf'], np.float64)[:, :, 3], axis=1)
    off = np.linalg.norm(np.asarray(rs['link_offset'], np.float64).reshape(L, 3), axis=1)
    frame = np.asarray(rs['link_frame']).astype(np.int64)
    rho = np.zeros((D, L), np.float64)
    for l in range(L):
        for i in range(min(D, int(frame[l]))):
            rho[i, l] = tl[i + 1:int(frame[l])].sum() + off[l]
    up = rho.astype(np.float32)
    low = up.astype(np.float64) < rho
    up[low] = np.nextafter(up[low], np.float32(np.inf))
    return up


def motion_bound(rs, rho, a, b):
    """Lambda (..., n_links) fp64 of the straight joint-space steps a -> b (..., n_dof): no collision sphere l moves farther than
    w Lambda_l while the parameter of the segment moves by w.  A chain: sum_i |b_i - a_i| rho_il; a point robot: |b - a|_2."""
    d = np.abs(np.asarray(b, np.float64) - np.asarray(a, np.float64))
    if int(rs['kind']) == 0:
        return np.sqrt((d * d).sum(-1))[..., None]
    return d @ np.asarray(rho, np.float64)


def pack_reach(rs):
    """The reach buffer of a robot spec as fp32 words (ints stored bit-exact): what ops.DeviceReach puts on the device."""
    rho = reach_table(rs)
    D, L = rho.shape
    if L > CERT_MAX_LINKS:
        raise ValueError(f'pack_reach: {L} collision spheres exceed CERT_MAX_LINKS = {CERT_MAX_LINKS}')
    buf = np.zeros(REACH_HEADER_WORDS + D * L, np.float32)
    buf.view(np.int32)[:REACH_HEADER_WORDS] = (REACH_MAGIC, D, L, int(rs['kind']))
    buf[REACH_HEADER_WORDS:] = rho.reshape(-1)
    return buf
