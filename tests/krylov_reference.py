"""
Host reference of the per-step kernels of the short-recurrence sibk (csrc/krylov.hip) and of the paired Gram-Schmidt
step (csrc/dense.hip: eigd_stack_cgs2_pair, eigd_pair_orthonormalise).  Plain numpy / Python, no GPU import, written from
the formulas in the header comment of krylov.hip and in include/eigd_hip.h:

    rr = r.z,  den = rr - alpha z.y,  gam = rr / den
    rho = 1 / (1 - (gam/gam') (rr/rr') / rho')               (primes: the state rows of the previous step; 1 in the first)
    r_new   = rho (r - gam (r - alpha y)) + (1 - rho) r_old
    psi_new = rho (psi + gam z)           + (1 - rho) psi_old

Everything is step-local: the expected state after a call is formed from exactly rounded inner products (math.fsum over
error-free products) and from the state the device itself held before the call, so rounding never makes two trajectories
drift apart and a tolerance is the rounding of ONE step.  tests/test_krylov_reference_cpu.py checks this module against
the solver of tests/test_cg_solution_cpu.py before tests/test_gpu_krylov_steps.py lets it judge a kernel.
"""
import math
from dataclasses import dataclass

import numpy as np

EPS = float(np.finfo(np.float64).eps) / 2.0      # unit roundoff of a double (2^-53)
LD = 64                                          # leading dimension of the state and log rows (kMaxK)
# rows of the state block in the enum order of krylov.hip (CgRow)
ROWS = {"rr": 0, "gam": 1, "rho": 2, "done": 3, "tol2": 4, "alpha": 5, "steps": 6, "flag": 7, "gam_now": 8, "rho_now": 9,
        "bad_rr": 10, "bad_den": 11, "bad_step": 12}
NROWS = len(ROWS)
BRANCHES = ("frozen-now", "frozen-before", "moves", "restart", "breakdown", "vanished")


def two_prod_terms(x, y):
    # Veltkamp / Dekker: x*y = p + e exactly, in pure Python floats
    out = []
    for a, b in zip(x.tolist(), y.tolist()):
        p = a * b
        sa = a * 134217729.0
        ah = sa - (sa - a)
        al = a - ah
        sb = b * 134217729.0
        bh = sb - (sb - b)
        bl = b - bh
        out += [p, ((ah * bh - p) + ah * bl + al * bh) + al * bl]
    return out


def _two_prod(X, Y):
    """the same split on whole arrays (IEEE double operations one by one, as above): (p, e) with X*Y = p + e exactly"""
    p = X * Y
    sa = X * 134217729.0
    ah = sa - (sa - X)
    al = X - ah
    sb = Y * 134217729.0
    bh = sb - (sb - Y)
    bl = Y - bh
    e = ((ah * bh - p) + ah * bl + al * bh) + al * bl
    return p, e


def exact_dots(X, Y):
    """(exactly rounded sum_i X[i,c] Y[i,c], sum_i |X[i,c] Y[i,c]|) per column of two n x k arrays"""
    X = np.ascontiguousarray(X, dtype=np.float64).reshape(len(X), -1)
    Y = np.ascontiguousarray(Y, dtype=np.float64).reshape(len(Y), -1)
    assert X.shape == Y.shape
    p, e = _two_prod(X, Y)
    pe = np.ascontiguousarray(np.concatenate([p, e], axis=0).T)
    k = X.shape[1]
    dots = np.array([math.fsum(pe[c].tolist()) for c in range(k)])
    # (a scale for error bounds: numpy's pairwise sum of positive numbers, good to 1e-15 relative; rounded up for good measure)
    sabs = np.abs(p).sum(axis=0) * (1.0 + 1e-12)
    return dots, sabs


@dataclass
class CoefStep:
    state: np.ndarray        # NROWS x k: the state block after the call
    log: np.ndarray          # 2 x k: rows 2 (step - 1) and 2 (step - 1) + 1 of the log
    branch: list             # per column, one of BRANCHES
    den: np.ndarray          # rr - alpha z.y (long double)
    q: np.ndarray            # 1 - (gam/gam')(rr/rr')/rho' where it was formed, else nan (long double)
    t: np.ndarray            # (gam/gam')(rr/rr')/rho' likewise


def coef_step(state_before, rz, zy, norm2, step, first):
    """
    What one call of the coefficient kernel leaves: state_before is the NROWS x k block the device held, rz / zy the exact
    inner products r.z and z.y per column, norm2 the squared residual norms the call is given (or None).
    """
    L = np.longdouble
    sb = np.array(state_before, dtype=np.float64)
    k = sb.shape[1]
    st = sb.copy()
    log = np.zeros((2, k))
    branch = []
    den = np.full(k, np.nan, dtype=L)
    qq = np.full(k, np.nan, dtype=L)
    tt = np.full(k, np.nan, dtype=L)
    R = ROWS
    for c in range(k):
        gam, rho = L(0.0), L(1.0)
        if sb[R["done"], c] != 0.0:
            branch.append("frozen-before")
        elif norm2 is not None and norm2[c] < sb[R["tol2"], c]:         # strictly below the tolerance
            st[R["done"], c] = 1.0
            st[R["steps"], c] = float(step - 1)
            branch.append("frozen-now")
        else:
            rr = L(rz[c])
            den[c] = rr - L(sb[R["alpha"], c]) * L(zy[c])
            if rr > 0 and den[c] > 0:
                gam = rr / den[c]
                name = "moves"
                if not first:
                    tt[c] = (gam / L(sb[R["gam"], c])) * (rr / L(sb[R["rr"], c])) / L(sb[R["rho"], c])
                    qq[c] = 1 - tt[c]
                    if qq[c] > 0:
                        rho = 1 / qq[c]
                    else:                                               # restart from the current iterate, counted once
                        name = "restart"
                        if sb[R["flag"], c] == 0.0:
                            st[R["flag"], c] = 1.0
                st[R["rr"], c], st[R["gam"], c], st[R["rho"], c] = float(rr), float(gam), float(rho)
                branch.append(name)
            elif rr != 0:
                if sb[R["flag"], c] != 2.0:                             # the record of the first breakdown stays
                    st[R["bad_rr"], c], st[R["bad_den"], c], st[R["bad_step"], c] = float(rr), float(den[c]), float(step)
                st[R["flag"], c] = 2.0
                branch.append("breakdown")
            else:
                branch.append("vanished")
        st[R["gam_now"], c] = log[0, c] = float(gam)
        st[R["rho_now"], c] = log[1, c] = float(rho)
    return CoefStep(st, log, branch, den, qq, tt)


def coef_bounds(cs, state_before, rz, s_rz, zy, s_zy, m):
    """
    Relative bounds (rr, gam, rho, den) per column on what a device evaluation of the step may deviate from `cs` by,
    when each inner product is a sum whose longest chain of additions is m (one more rounding for the product):
        |rz_dev - rz| <= g s_rz,   |zy_dev - zy| <= g s_zy,   g = (m + 1) u / (1 - (m + 1) u)
        den = rr - alpha zy (two more roundings, or one fused): |d den| <= g s_rz + |alpha| g s_zy + 2 u (|rr| + |alpha zy|)
        gam = rr / den:            e_gam <= e_rr + e_den + u              (first order, the 1.01 below covers the rest)
        t = (gam/gam')(rr/rr')/rho' with the primes exact: e_t <= e_gam + e_rr + 4 u
        q = 1 - t:                 |dq| <= |t| e_t + u |q|;   rho = 1/q:  e_rho <= |dq| / |q| + u
    """
    u = EPS
    g = (m + 1) * u / (1.0 - (m + 1) * u)
    sb = np.asarray(state_before, dtype=np.float64)
    al = np.abs(sb[ROWS["alpha"]])
    rr = np.abs(np.asarray(rz, dtype=np.float64))
    den = np.abs(cs.den.astype(np.float64))
    with np.errstate(divide="ignore", invalid="ignore"):
        e_rr = g * s_rz / rr
        e_den = (g * s_rz + al * g * s_zy + 2 * u * (rr + al * np.abs(zy))) / den
        e_gam = e_rr + e_den + u
        e_t = e_gam + e_rr + 4 * u
        t, q = np.abs(cs.t.astype(np.float64)), np.abs(cs.q.astype(np.float64))
        e_rho = (t * e_t + u * q) / q + u
    return 1.01 * e_rr, 1.01 * e_gam, 1.01 * e_rho, 1.01 * e_den


def update_step(r, r_old, psi, psi_old, z, y, gam, rho, alpha, first):
    """
    (r_new, sum of |terms| of r_new, psi_new, sum of |terms| of psi_new), n x k each: the values in long double, the
    sums of absolute values (scales of error bounds) in double.  gam[c] == 0: the
    column does not move (a copy); first, or rho[c] == 1: the two-term step, r_old / psi_old are not looked at; z and y
    are not looked at in a column that does not move.  psi None: the residual alone (psi_new and its terms are None).
    """
    L = np.longdouble
    n, k = r.shape
    rn, ra = np.empty((n, k), dtype=L), np.empty((n, k))
    with_psi = psi is not None
    pn = np.empty((n, k), dtype=L) if with_psi else None
    pa = np.empty((n, k)) if with_psi else None
    for c in range(k):
        r64 = r[:, c]
        rv = r64.astype(L)
        s64 = psi[:, c] if with_psi else None
        sv = s64.astype(L) if with_psi else None
        g, rh, al = L(gam[c]), L(rho[c]), L(alpha[c])
        g64, rh64, al64 = abs(float(gam[c])), float(rho[c]), abs(float(alpha[c]))
        if g == 0:
            rn[:, c], ra[:, c] = rv, np.abs(r64)
            if with_psi:
                pn[:, c], pa[:, c] = sv, np.abs(s64)
            continue
        a = rv - g * (rv - al * y[:, c].astype(L))
        aa = np.abs(r64) + g64 * (np.abs(r64) + al64 * np.abs(y[:, c]))
        if with_psi:
            b = sv + g * z[:, c].astype(L)
            ba = np.abs(s64) + g64 * np.abs(z[:, c])
        if not first and rh != 1:
            a, aa = rh * a + (1 - rh) * r_old[:, c].astype(L), abs(rh64) * aa + abs(1.0 - rh64) * np.abs(r_old[:, c])
            if with_psi:
                b, ba = rh * b + (1 - rh) * psi_old[:, c].astype(L), abs(rh64) * ba + abs(1.0 - rh64) * np.abs(psi_old[:, c])
        rn[:, c], ra[:, c] = a, aa * (1.0 + 1e-12)
        if with_psi:
            pn[:, c], pa[:, c] = b, ba * (1.0 + 1e-12)
    return rn, ra, pn, pa


def cgs2_pair_ref(S, T):
    """
    S: ns slabs of n x k; T = [T1 | T2], n x 2k.  Column c of T1 and column c of T2 both meet column c of every slab.
    Returns (H, T_new): H[j] = [S_j . T1 | S_j . T2] (ns x 2k) and T_new = T - sum_j S_j H[j], in long double.
    """
    L = np.longdouble
    k = S[0].shape[1]
    assert T.shape[1] == 2 * k
    TL = T.astype(L)
    H = np.empty((len(S), 2 * k), dtype=L)
    Tn = TL.copy()
    for j, Sj in enumerate(S):
        SL = np.concatenate([Sj, Sj], axis=1).astype(L)
        H[j] = (SL * TL).sum(axis=0)
        Tn -= SL * H[j]
    return H, Tn


def pair_orthonormalise_ref(T, norm2, skip):
    """
    T = [T1 | T2] (n x 2k), norm2 the squared column norms of T1 as the call is given them, skip a mask of k columns:
        W1 = T1 / |T1|,  T2' = T2 - (T1.T2 / |T1|^2) T1,  W2 = T2' / |T2'|,
        out = [ |T1|^2 | T1.T2 | |T2'|^2 | W1.T2' ]                        (long double)
    A column that is skipped or has norm2 == 0 gives W1 = T2' = W2 = 0 and zeros in the last two groups; |T2'| == 0
    gives W2 = 0.
    """
    L = np.longdouble
    k = T.shape[1] // 2
    T1, T2 = T[:, :k].astype(L), T[:, k:2 * k].astype(L)
    n1 = np.asarray(norm2, dtype=np.float64)[:k].astype(L)
    gamma = (T1 * T2).sum(axis=0)
    dead = np.asarray(skip, dtype=bool)[:k] | (n1 == 0)
    safe = np.where(dead, L(1), n1)
    W1 = np.where(dead, L(0), T1 / np.sqrt(safe))
    T2n = np.where(dead, L(0), T2 - (gamma / safe) * T1)
    n2 = (T2n * T2n).sum(axis=0)
    d = (W1 * T2n).sum(axis=0)
    dead2 = dead | (n2 == 0)
    W2 = np.where(dead2, L(0), T2n / np.sqrt(np.where(dead2, L(1), n2)))
    return W1, T2n, W2, np.concatenate([n1, gamma, n2, d])


# ---- the launch geometry of the kernels (what the longest chain of additions of a sum is) -----------------------------

def next_pow2(k):
    p = 1
    while p < k:
        p *= 2
    return p


def cg_geometry(n, k, rows_per_thread):
    """(workgroups, RP, rows a thread walks) of cg_dots_kernel (8 rows per thread) / cg_update_kernel (4): 256 threads,
    KP = next power of two of k columns, RP = 256 / KP rows per trip, at most 1024 workgroups with a grid-stride loop"""
    rp = 256 // next_pow2(k)
    nb = max(1, min(-(-n // (rp * rows_per_thread)), 1024))
    return nb, rp, -(-n // (nb * rp))


def cg_chain(n, k, rows_per_thread):
    """longest chain of additions one term of a column sum goes through"""
    nb, rp, per_thread = cg_geometry(n, k, rows_per_thread)
    # per-thread rows + the RP sum of the workgroup + the lane's walk over the partials (every 64th) + 6 shuffle levels
    return per_thread + rp + -(-nb // 64) + 6


# ---- crafted inputs for the branches of the coefficient kernel --------------------------------------------------------

def blank_state(k, alpha, tol2=1e-30):
    st = np.zeros((NROWS, k))
    st[ROWS["tol2"]] = tol2
    st[ROWS["alpha"]] = alpha
    return st


def branch_case(name, n=1000, k=6):
    """
    One crafted situation of the coefficient kernel: a dict with `state` (NROWS x k, before the first call) and `calls`,
    a list of dicts (R, Z, Y, norm2 or None, step, first, expect: the branch of every column).  All data are seeded
    normals with distinct columns; z = f r with f > 0 and y = g z with g > 0 unless the case says otherwise, so that
    r.z > 0 and z.y > 0 with no cancellation.
    """
    rng = np.random.default_rng(sum(map(ord, name)))
    R = rng.normal(size=(n, k))
    f, g = rng.uniform(0.5, 2.0, size=(n, k)), rng.uniform(0.5, 2.0, size=(n, k))
    Z = f * R
    Y = g * Z
    alpha = -rng.uniform(0.1, 0.5, size=k)
    st = blank_state(k, alpha)
    rr = np.sum(R * Z, axis=0)

    def call(step, first, expect, R=R, Z=Z, Y=Y, norm2=None):
        return {"R": R, "Z": Z, "Y": Y, "norm2": norm2, "step": step, "first": first, "expect": list(expect)}

    if name == "restart":
        # the previous r.z is tiny against this step's (it "has grown by orders"): (gam/gam')(rr/rr')/rho' ~ 1e30, q < 0
        st[ROWS["gam"]], st[ROWS["rho"]] = 0.9, 1.1
        st[ROWS["rr"]] = 1e-30 * rr
        st[ROWS["rr"], 3] = 4.0 * rr[3]               # an ordinary step in between
        st[ROWS["flag"], 1], st[ROWS["flag"], 2] = 2.0, 1.0   # flags that are already set stay what they are
        exp = ["restart"] * k
        exp[3] = "moves"
        return {"state": st, "calls": [call(5, 0, exp)]}
    if name in ("den", "rr_neg"):
        if name == "den":                             # alpha > 0, large against a positive z.y: rr - alpha z.y < 0
            st[ROWS["alpha"]] = 1e3
            Z1, Y1 = Z, Y
        else:                                         # z = -f r: r.z < 0
            Z1 = -Z
            Y1 = g * Z1
        st[ROWS["rr"]], st[ROWS["gam"]], st[ROWS["rho"]] = 3.0 + np.arange(k), 0.7, 1.2    # must stay
        st[ROWS["alpha"], 0] = alpha[0]
        st[ROWS["rr"], 0] = 4.0 * rr[0]
        exp = ["breakdown"] * k
        exp[0] = "moves"                              # column 0 (alpha < 0, z = f r): an ordinary step next to the breakdowns
        if name == "den":
            Zc, Yc = Z1, Y1
        else:
            Zc, Yc = Z1.copy(), Y1.copy()
            Zc[:, 0], Yc[:, 0] = Z[:, 0], Y[:, 0]
        R2 = 0.5 * R                                  # the second occurrence sees other numbers and another step
        Z2 = f * R2 if name == "den" else np.concatenate([(f * R2)[:, :1], -(f * R2)[:, 1:]], axis=1)
        return {"state": st, "calls": [call(4, 0, exp, Z=Zc, Y=Yc), call(7, 0, exp, R=R2, Z=Z2, Y=g * Z2)]}
    if name == "vanished":
        R0, Z0, Y0 = R.copy(), Z.copy(), Y.copy()
        R0[:, 2] = Z0[:, 2] = Y0[:, 2] = 0.0
        exp = ["moves"] * k
        exp[2] = "vanished"
        return {"state": st, "calls": [call(1, 1, exp, R=R0, Z=Z0, Y=Y0)]}
    if name == "frozen":
        tol2 = 10.0 ** -np.arange(3, 3 + k)
        st[ROWS["tol2"]] = tol2
        norm2 = 8.0 * tol2                            # above: moves
        norm2[1] = 0.5 * tol2[1]                      # below: frozen in this step
        norm2[2] = tol2[2]                            # equal: the comparison is strict, the column moves
        st[ROWS["done"], 3], st[ROWS["steps"], 3] = 1.0, 2.0   # frozen earlier: stays, whatever the norm says now
        norm2[3] = 1e6
        norm2[4] = np.nextafter(tol2[4], 0.0)         # the last double below the tolerance
        st[ROWS["gam"]], st[ROWS["rho"]], st[ROWS["rr"]] = 0.9, 1.1, 4.0 * rr
        exp = ["moves"] * k
        exp[1], exp[3], exp[4] = "frozen-now", "frozen-before", "frozen-now"
        return {"state": st, "calls": [call(6, 0, exp, norm2=norm2)]}
    raise KeyError(name)


BRANCH_CASES = ("restart", "den", "rr_neg", "vanished", "frozen")
