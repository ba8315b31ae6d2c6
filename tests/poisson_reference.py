"""numpy's Poisson draw (``random_poisson`` of numpy/random/src/distributions/distributions.c) restated over the raw 64-bit outputs of the bit
generator in plain Python floats -- IEEE doubles in numpy's order, no contraction, ``math.log`` / ``math.exp`` / ``math.sqrt``, the functions
numpy's C code calls -- with the consumption and the branch of every draw, the window scheme of pyimcom_amd/csrc/poisson_core.h (the least
consumption, the drift, the window's lower edge) restated beside it, and searches over seeds for named events."""

import math

import numpy as np

ZERO, MULT, PTRS = 0, 1, 2  # the branch of a draw
UNDECIDED, OVERCAP = 1, 2  # flags
PTRS_CAP, MULT_CAP, HALO = 32, 64, 64
GUARD = 2.0**-47
LAM_MAX = 9.223372006484771e18
LOGGAM_A = (8.333333333333333e-02, -2.777777777777778e-03, 7.936507936507937e-04, -5.952380952380952e-04, 8.417508417508418e-04,
            -1.917526917526918e-03, 6.410256410256410e-03, -2.955065359477124e-02, 1.796443723688307e-01, -1.39243221690590e00)
# the outcome of a PTRS attempt
FAST, QUICK_REJECT, SLOW_ACCEPT, SLOW_REJECT = "fast", "quick_reject", "slow_accept", "slow_reject"


def uniform(w):
    return (int(w) >> 11) * 2.0**-53


def loggam(x):
    """(numpy's random_loggam(x), the summed magnitudes of its terms)."""
    if x == 1.0 or x == 2.0:
        return 0.0, 0.0
    n = int(7 - x) if x < 7.0 else 0
    x0 = x + n
    x2 = (1.0 / x0) * (1.0 / x0)
    lg2pi = 1.8378770664093453e00
    gl0 = LOGGAM_A[9]
    for k in range(8, -1, -1):
        gl0 *= x2
        gl0 += LOGGAM_A[k]
    t0, t1, t2 = gl0 / x0, 0.5 * lg2pi, (x0 - 0.5) * math.log(x0)
    gl = t0 + t1 + t2 - x0
    mag = abs(t0) + t1 + abs(t2) + x0
    if x < 7.0:
        for _ in range(1, n + 1):
            lg = math.log(x0 - 1.0)
            gl -= lg
            mag += abs(lg)
            x0 -= 1.0
    return gl, mag


def draw(lam, raw, p, guard=0.0):
    """(value, outputs consumed, branch, flags, outcomes) of the draw of rate ``lam`` that starts at raw[p]; raw: Python ints.  outcomes: one
    entry per PTRS attempt.  A comparison within the guard band (poisson_core.h) sets UNDECIDED and is then decided as it stands."""
    lam = float(lam)
    if not lam > 0.0:
        return 0, 0, ZERO, 0, ()
    if lam < 10.0:
        enlam, prod, flags = math.exp(-lam), 1.0, 0
        for t in range(MULT_CAP):
            prod *= uniform(raw[p + t])
            if abs(prod - enlam) <= guard * enlam:
                flags |= UNDECIDED
            if not prod > enlam:
                return t, t + 1, MULT, flags, ()
        return MULT_CAP, MULT_CAP, MULT, flags | OVERCAP, ()
    slam, loglam = math.sqrt(lam), math.log(lam)
    b = 0.931 + 2.53 * slam
    a = -0.059 + 0.02483 * b
    invalpha = 1.1239 + 1.1328 / (b - 3.4)
    vr = 0.9277 - 3.6224 / (b - 2)
    flags, outcomes = 0, []
    for t in range(PTRS_CAP):
        U, V = uniform(raw[p + 2 * t]) - 0.5, uniform(raw[p + 2 * t + 1])
        us = 0.5 - abs(U)
        if us == 0.0:  # (2^-53 of the attempts: the division is infinite in C)
            outcomes.append(QUICK_REJECT)
            if V > us:
                continue
            return 0, 2 * t + 2, PTRS, flags | UNDECIDED, tuple(outcomes)
        kf = math.floor((2 * a / us + b) * U + lam + 0.43)
        if us >= 0.07 and V <= vr:
            outcomes.append(FAST)
            return int(kf), 2 * t + 2, PTRS, flags, tuple(outcomes)
        if kf < 0 or (us < 0.013 and V > us):
            outcomes.append(QUICK_REJECT)
            continue
        l0 = math.log(V) if V > 0.0 else -math.inf
        l1, l2, kl = math.log(invalpha), math.log(a / (us * us) + b), float(kf) * loglam
        lg, mag = loggam(float(kf + 1))
        mag += abs(l0) + abs(l1) + abs(l2) + lam + abs(kl)
        lhs, rhs = l0 + l1 - l2, -lam + kl - lg
        if not abs(lhs - rhs) > guard * mag:
            flags |= UNDECIDED
        if lhs <= rhs:
            outcomes.append(SLOW_ACCEPT)
            return int(kf), 2 * t + 2, PTRS, flags, tuple(outcomes)
        outcomes.append(SLOW_REJECT)
    return 0, 2 * PTRS_CAP, PTRS, flags | OVERCAP, tuple(outcomes)


def poisson_from_raw(raw, lam, guard=0.0):
    """The draws of the rates ``lam`` (any shape, C order) from raw[0] on: a dict of ``values`` int64 [n], ``adv`` (outputs each draw
    consumed), ``pos`` (where each started), ``branch``, ``flags``, ``outcomes`` (per draw, the PTRS attempts) and ``consumed``."""
    lam = np.asarray(lam, dtype=np.float64).ravel()
    raw = [int(w) for w in np.asarray(raw, dtype=np.uint64)]
    n = lam.size
    out = dict(values=np.zeros(n, np.int64), adv=np.zeros(n, np.int64), pos=np.zeros(n, np.int64), branch=np.zeros(n, np.int64),
               flags=np.zeros(n, np.int64), outcomes=[()] * n)
    p = 0
    for i, lm in enumerate(lam.tolist()):
        if p + HALO > len(raw):
            raise ValueError("not enough outputs")
        v, adv, branch, flags, outcomes = draw(lm, raw, p, guard)
        out["values"][i], out["adv"][i], out["pos"][i], out["branch"][i], out["flags"][i] = v, adv, p, branch, flags
        out["outcomes"][i] = outcomes
        p += adv
    out["consumed"] = p
    return out


def raw_for(seed, lam, offset=0):
    """Outputs of PCG64(seed) from ``offset`` on, enough for the rates ``lam``."""
    lam = np.asarray(lam, dtype=np.float64).ravel()
    bg = np.random.PCG64(seed)
    if offset:
        bg.advance(offset)
    room = int(np.sum(np.where(lam >= 10.0, 3.0, 2.0 * lam + 2.0))) + 64 * int(np.sqrt(lam.size) + 1) + 4 * HALO
    return bg.random_raw(room)


# ---- the window scheme of poisson_core.h ---------------------------------------------------------------------------------------------------
DRIFT_TAB = (0.2480, 0.2853, 0.3260, 0.3702, 0.4181, 0.4708, 0.5288, 0.5934, 0.6646)


def min_adv(lam):
    return 0 if not lam > 0.0 else (1 if lam < 10.0 else 2)


def drift256(lam):
    if not lam > 0.0:
        return 0
    if lam < 10.0:
        return int(lam * 256.0)
    x = 25.0 / math.sqrt(lam)
    i = 7 if x >= 7.0 else int(x)
    return int(256.0 * (DRIFT_TAB[i] + (DRIFT_TAB[i + 1] - DRIFT_TAB[i]) * (x - i)) + 0.5)


def window_lo(D, W):
    return max(0, (D >> 8) - W // 2)


def windows(raw, lam, S, W, guard=0.0):
    """What the table path of poisson.hip sees for superchunks of S draws and windows of W excesses: per superchunk ``leaves`` (the path
    leaves a window), ``on_path`` (flags of the path's draws) and ``off_path`` (window nodes off the path with a flag)."""
    lam = np.asarray(lam, dtype=np.float64).ravel().tolist()
    path = poisson_from_raw(raw, lam, guard)
    rawl = [int(w) for w in np.asarray(raw, dtype=np.uint64)]
    res = []
    for s0 in range(0, len(lam), S):
        ns = min(S, len(lam) - s0)
        p0, mb, D = int(path["pos"][s0]), 0, 0
        leaves, on_path, off_path = False, 0, 0
        for j in range(ns):
            lm, lo = lam[s0 + j], window_lo(D, W)
            x = int(path["pos"][s0 + j]) - p0 - mb
            adv = int(path["adv"][s0 + j])
            if not lo <= x < lo + W or (path["branch"][s0 + j] == PTRS and (x - lo + adv - 2 >= W or adv >= 2 * PTRS_CAP)):
                leaves = True  # (a PTRS node is resolved attempt by attempt inside the window: poi_node_leaves of poisson_core.h)
            on_path |= int(path["flags"][s0 + j])
            for w in range(W):
                if lo + w != x and draw(lm, rawl, p0 + mb + lo + w, guard)[3]:
                    off_path += 1
            mb += min_adv(lm)
            D += drift256(lm)
        res.append(dict(leaves=leaves, on_path=on_path, off_path=off_path))
    return res


def find_seed(lam, wanted, start=0, limit=100000, offset=0):
    """The first seed >= start for which ``wanted(poisson_from_raw(...))`` holds for the rates ``lam``; None after ``limit`` seeds."""
    for seed in range(start, start + limit):
        if wanted(poisson_from_raw(raw_for(seed, lam, offset), lam)):
            return seed
    return None


def rejected_at(index):
    """wanted(): draw ``index`` takes more than one attempt (its second attempt starts inside the draw)."""
    return lambda r: len(r["outcomes"][index]) >= 2


def slow_at(index, accept):
    """wanted(): the last attempt of draw ``index`` is a slow-test accept; or (accept False) the draw holds a slow-test reject."""
    if accept:
        return lambda r: len(r["outcomes"][index]) >= 1 and r["outcomes"][index][-1] == SLOW_ACCEPT
    return lambda r: SLOW_REJECT in r["outcomes"][index]


def mult_at_least(index, x):
    return lambda r: r["branch"][index] == MULT and r["values"][index] >= x
