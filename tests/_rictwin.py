"""The pin of the Riccati backward sweep (k_ric_bwd / k_ric_bwd4 in hb_kernels.hip, ric_phase12 / ric_phase3_* / ric_factor_solve in
hb_riccati.hpp), stage by stage, numpy only: twelve cases in one context of B = 12 instances and Nmax = 24 stages, a reference of the
recursion of SURVEY.md B.5 in numpy.longdouble, and check(), which the host runner (tests/test_riccati_pin_host.py, host emulator) and
the device runner (tests/test_gpu_riccati_pin.py, both forms of the sweep and the automatic choice) share.  The code under test is
entered through hb_riccati_gains (include/hunter_hip.h) or its host twin emu_riccati_gains (tests/host_emu/hostemu.cpp).

Reference.  Huu = R + B'SB, Hux = P + B'SA, hu = r + B'(Sb + s), K = -Huu^-1 Hux, k = -Huu^-1 hu, s <- q + A'(Sb + s) + Hux'k,
S <- sym(Q + A'SA + Hux'K), S_N = 0, on the real widths only, solved by Cholesky, in numpy.longdouble (64-bit mantissa, asserted).
tests/test_riccati_pin_host.py validates it against mpmath at 40 digits on every case: its distance from mpmath must stay below a
thousandth of every bound it is used for.

Cases (a case is an instance; widths in sweep order, last stage first).  Problems are drawn like test_riccati's (A = I + 0.05 noise,
B = 0.1 noise, b = 0.01 noise, Q, R = M M' + 0.5 I, P = 0.05 noise, q, r noise) unless said otherwise.
   0  N  1  9                        one stage: the first fetch and the re-request of the own record coincide
   1  N  2  12, 6                    shortest wide -> narrow hand-over
   2  N 24  all 12                   N = Nmax, tail block every stage
   3  N 17  WIDTHS3 repeating        every ordered pair of widths adjacent; (n_f, n_z) split as (6, 3), (9, 0), (6, 0), (12, 0), (9, 3)
   4  N 17  all 6                    padded factor rows 6..8
   5  N 16  all 9, c = 1e6           conditioning
   6  N 16  all 12, c = 1e10         conditioning through ric_factor_tail
   7  N 16  as 3, A = I + 0.3 noise  S grows over the horizon
   8  N  5  all 9                    stage 2 indefinite: flag in the leading block
   9  N  5  all 12                   stage 2 indefinite only in rows 9..11: flag in the tail block
  10  N 17  copy of 3                position independence
  11  N  3  6, 12, 6                 widths change both ways around one stage; rotation role 3 of the four-wavefront form
WIDTHS3 = 12, 9, 6, 9, 9, 12, 12, 6, 6.  (A cycle of nine stages holds each of the nine ordered pairs exactly once only if it is an
Euler circuit of the pair graph; 12, 9, 6, 9, 12, 12, 6, 6, 9 is none: it lacks (9, 9) and (6, 12).  The builder asserts the nine pairs.)
Conditioned cases (5, 6).  R = V diag(logspace(0, -log10 c)) V' with a random orthogonal V.  With B and P drawn as above, B'SB (S >= Q >=
0.5 I) would lift every eigenvalue of Huu = R + B'SB to ~1e-2 at all stages but the last, and Q - P'R^-1 P would be indefinite by ~1e-3 c
there.  So these cases draw B0, P0 as above and use B = B0 R^1/2, P = R^1/2 P0: Huu = R^1/2 (I + B0'SB0) R^1/2 keeps the spectrum of R
at every stage and the stage cost stays positive definite (Q - P0'P0 > 0).  An unpivoted factorisation sees the full conditioning.
Flag cases (8, 9).  Stage 2 has R = V diag(..., -20) V' (case 9: V = blkdiag(V9, V3), the negative eigenvalue in the 3 x 3 block, so
that the leading 9 x 9 block of Huu is positive definite and the pivot that fails lies in rows 9..11).

Conditions the builder asserts from the reference alone (cases()): on non-flag cases every pivot of the root-free factorisation of
Huu_ref is positive with smallest / largest >= 1e-12; on flag cases the offending pivot is negative with magnitude >= 1e-6 of the
largest (the decision is not a matter of rounding) and lies in the block the case is for; case 3 holds all nine ordered width pairs and
all five (n_f, n_z) splits.

check(K, k, ric_fail, what):
  structure, exact   rows >= n_f + n_z of K~, k~ of every stage are exactly zero; every gain slot of a stage k >= N[i] holds the
                     sentinel bit for bit; ric_fail is 1 for cases 8 and 9 and 0 elsewhere; case 10 equals case 3 bit for bit;
  forward error      max|K~ - K_ref| / max(1, max|K_ref|) and the same for k~, per stage;
  backward error     |Huu_ref K~ + Hux_ref|_inf / (|Huu_ref|_inf |K~|_inf + |Hux_ref|_inf) and the same with hu, k~, per stage (it does
                     not loosen with cond(Huu));
on cases 8 and 9 the last two only on the stages behind the failing one in sweep order (k > 2).
Bounds, per case and figure: 8 x the largest distance from the reference of three plain float64 evaluations of the same recursion
(LAPACK Cholesky, numpy.linalg.solve, a root-free U D U' in Python loops; worst stage) + 32 x 2^-53.  The family and not one member:
its members lie a factor of up to 50 apart on the conditioned cases.  8 is the project's margin for "device against the twin's
distance" (tests/_primcheck.py).  A figure over its bound is a finding about the code, not a reason to raise the factor.

Measured worst ratio (distance / bound) per case, over the four figures and all held stages; the forward distance of K~ of the
float64 family (best .. worst member) next to it.  k_ric_bwd, k_ric_bwd4 and the automatic choice give identical bits, hence one column.
  case   family, forward K~     host emulator   device, either form
    0    5.2e-17 .. 6.2e-17         0.05              0.05
    1    5.5e-16 .. 6.0e-16         0.16              0.16
    2    1.3e-15 .. 1.5e-15         0.10              0.10
    3    9.8e-16 .. 1.7e-15         0.09              0.09
    4    9.9e-16 .. 1.3e-15         0.09              0.10
    5    7.2e-11 .. 1.1e-10         0.16              0.09
    6    4.4e-07 .. 8.5e-07         0.33              0.19
    7    5.7e-15 .. 1.0e-14         0.15              0.12
    8    6.5e-16 .. 8.0e-16         0.14              0.10
    9    4.7e-16 .. 9.2e-16         0.10              0.09
   10    as 3                       0.09              0.09
   11    8.6e-16 .. 1.0e-15         0.09              0.11
The long-double reference lies at most 1.3e-4 of a bound from mpmath (case 6: backward error of K~ 5.6e-16 against a bound of 4.6e-12,
forward 4.1e-10 against 6.8e-6, where the float64 family sits at 4.4e-7 .. 8.5e-7).
"""
import functools

import numpy as np

B, NMAX, NCASES = 12, 24, 12
SENTINEL_BITS = np.uint64(0x7ff85e471e100001)        # HB_RIC_GAINS_SENTINEL_BITS (include/hunter_hip.h)
WIDTHS3 = (12, 9, 6, 9, 9, 12, 12, 6, 6)
SPLITS = {6: ((6, 0),), 9: ((6, 3), (9, 0)), 12: ((12, 0), (9, 3))}
FLAG_CASES, FLAG_STAGE = (8, 9), 2
FIGURES = ("forward error of K", "forward error of k", "backward error of K", "backward error of k")
FACTOR, FLOOR = 8.0, 32 * 2.0 ** -53
LD = np.longdouble


# ------------------------------------------------------------------------------------------------------------------ cases
def _orth(rng, n):
    q, r = np.linalg.qr(rng.standard_normal((n, n)))
    return q * np.sign(np.diag(r))


def _sym(m):
    return 0.5 * (m + m.T)


def _spd(rng, n):
    m = rng.standard_normal((n, n))
    return _sym(m @ m.T + 0.5 * np.eye(n))


def _draw(seed, sweep_widths, a_noise=0.05, cond=None, indefinite=None):
    """One instance: per stage k (time order) a dict of A, B, b, Q, R, P, q, r at the stage's real width nu, and (n_f, n_z)."""
    rng = np.random.default_rng(seed)
    N = len(sweep_widths)
    turn = {6: 0, 9: 0, 12: 0}
    stages = [None] * N
    for j, nu in enumerate(sweep_widths):
        k = N - 1 - j
        split = SPLITS[nu][turn[nu] % len(SPLITS[nu])]
        turn[nu] += 1
        st = dict(nu=nu, n_f=split[0], n_z=split[1], A=np.eye(22) + a_noise * rng.standard_normal((22, 22)),
                  B=0.1 * rng.standard_normal((22, nu)), b=0.01 * rng.standard_normal(22), Q=_spd(rng, 22), R=_spd(rng, nu),
                  P=0.05 * rng.standard_normal((nu, 22)), q=rng.standard_normal(22), r=rng.standard_normal(nu))
        if cond is not None:
            V, lam = _orth(rng, nu), np.logspace(0.0, -np.log10(cond), nu)
            root = _sym((V * np.sqrt(lam)) @ V.T)
            st["R"], st["B"], st["P"] = _sym((V * lam) @ V.T), st["B"] @ root, root @ st["P"]
        if indefinite is not None and k == FLAG_STAGE:
            lam = np.linspace(1.0, 2.0, nu)
            lam[-1] = -20.0
            if indefinite == "tail":
                V = np.zeros((nu, nu))
                V[:9, :9], V[9:, 9:] = _orth(rng, 9), _orth(rng, nu - 9)
            else:
                V = _orth(rng, nu)
            st["R"] = _sym((V * lam) @ V.T)
        stages[k] = st
    return stages


def _sweep3(N):
    return [WIDTHS3[j % len(WIDTHS3)] for j in range(N)]


def _pairs(widths):
    return {(a, b) for a, b in zip(widths[:-1], widths[1:])}


@functools.lru_cache(None)
def _data():
    """the twelve instances (lists of stage dicts, time order)"""
    assert np.finfo(LD).eps < 2e-19, "numpy.longdouble has no 64-bit mantissa here: the reference would not be better than what it judges"
    c = [
        _draw(100, [9]), _draw(101, [12, 6]), _draw(102, [12] * 24), _draw(103, _sweep3(17)), _draw(104, [6] * 17),
        _draw(105, [9] * 16, cond=1e6), _draw(106, [12] * 16, cond=1e10), _draw(107, _sweep3(16), a_noise=0.3),
        _draw(108, [9] * 5, indefinite="lead"), _draw(109, [12] * 5, indefinite="tail"), _draw(103, _sweep3(17)), _draw(111, [6, 12, 6]),
    ]
    assert len(c) == NCASES <= B and all(1 <= len(x) <= NMAX for x in c)
    return c


@functools.lru_cache(None)
def cases():
    """_data() with the conditions of the docstring asserted, from the reference alone.  No case may be skipped."""
    c = _data()
    sweep = [st["nu"] for st in reversed(c[3])]
    assert _pairs(sweep) == {(a, b) for a in (6, 9, 12) for b in (6, 9, 12)}, "case 3 must hold all nine ordered width pairs"
    assert {(st["n_f"], st["n_z"]) for st in c[3]} == {(6, 3), (9, 0), (6, 0), (12, 0), (9, 3)}
    for a, b in zip(c[3], c[10]):
        assert all(np.array_equal(a[key], b[key]) for key in "ABbQRPqr") and (a["n_f"], a["n_z"]) == (b["n_f"], b["n_z"])
    for i, ref in enumerate(reference()):
        assert sorted(ref["pivots"]) == list(range(FLAG_STAGE if i in FLAG_CASES else 0, len(c[i])))
        for k, d in ref["pivots"].items():
            if i in FLAG_CASES and k == FLAG_STAGE:
                j = int(np.argmax(d <= 0))
                assert d[j] < 0 and (d[:j] > 0).all() and -d[j] >= 1e-6 * np.abs(d).max(), f"case {i}: the offending pivot {d[j]} of {d}"
                assert (j >= 9) == (i == 9), f"case {i}: the pivot that fails lies in row {j}"
            else:
                assert (d > 0).all() and d.min() / d.max() >= 1e-12, f"case {i} stage {k}: pivots {d}"
    return c


# ------------------------------------------------------------------------------------------------------------------ the recursion
def _ldl_pivots(H):
    """pivots d of the root-free factorisation H = U D U' (U unit lower triangular, no pivoting), in the arithmetic of H"""
    H = H.copy()
    n = H.shape[0]
    d = np.zeros(n, dtype=H.dtype)
    for j in range(n):
        d[j] = H[j, j]
        if d[j] == 0:
            break
        col = H[j + 1:, j].copy()
        H[j + 1:, j + 1:] -= np.outer(col, col) / d[j]
    return d


def _subst(L, rhs, sqrt):
    """L L' x = rhs by two substitutions, in the arithmetic of L"""
    n = L.shape[0]
    y = rhs.copy()
    for i in range(n):
        y[i] = (y[i] - L[i, :i] @ y[:i]) / L[i, i]
    for i in range(n - 1, -1, -1):
        y[i] = (y[i] - L[i + 1:, i] @ y[i + 1:]) / L[i, i]
    return y


def solve_cholesky_loops(H, rhs, sqrt=np.sqrt):
    """Cholesky in loops, in whatever arithmetic the arrays carry (numpy.longdouble: the reference; mpmath objects: its validation)"""
    n = H.shape[0]
    L = np.zeros_like(H)
    for j in range(n):
        v = H[j, j] - L[j, :j] @ L[j, :j]
        assert v > 0, "the reference met a pivot that is not positive"
        L[j, j] = sqrt(v)
        for i in range(j + 1, n):
            L[i, j] = (H[i, j] - L[i, :j] @ L[j, :j]) / L[j, j]
    return _subst(L, rhs, sqrt)


def solve_lapack_cholesky(H, rhs):
    return _subst(np.linalg.cholesky(H), rhs, np.sqrt)


def solve_lu(H, rhs):
    return np.linalg.solve(H, rhs)


def solve_udu_loops(H, rhs):
    """root-free U D U' in Python loops, float64: right-looking elimination, reciprocal pivots, z = U^-1 b, w = z / d, y = U'^-1 w"""
    n = H.shape[0]
    L = np.tril(H).copy()
    rd = np.zeros(n)
    for j in range(n):
        rd[j] = 1.0 / L[j, j]
        for i in range(j + 1, n):
            t = L[i, j]
            for m in range(j + 1, i):
                L[i, m] -= t * L[m, j]
            L[i, i] -= t * t * rd[j]
            L[i, j] = t * rd[j]
    y = rhs.copy()
    for a in range(n):
        for m in range(a):
            y[a] = y[a] - L[a, m] * y[m]
    for a in range(n - 1, -1, -1):
        y[a] = y[a] * rd[a]
        for m in range(a + 1, n):
            y[a] = y[a] - L[m, a] * y[m]
    return y


def recursion(stages, convert, solve, stop_at=None, zero=0.0):
    """The recursion of SURVEY.md B.5 over one instance in the arithmetic `convert` puts the data into.  -> {k: dict(K, k, Huu, Hux,
    hu)} for the stages computed; at stage `stop_at` only Huu is formed (its solve is what the flag cases must not do)."""
    S = convert(np.zeros((22, 22)))
    s = convert(np.zeros(22))
    out = {}
    for k in range(len(stages) - 1, -1, -1):
        st = {key: convert(stages[k][key]) for key in "ABbQRPqr"}
        SA, SB, Sb = S @ st["A"], S @ st["B"], S @ st["b"] + s
        Huu, Hux, hu = st["R"] + st["B"].T @ SB, st["P"] + st["B"].T @ SA, st["r"] + st["B"].T @ Sb
        if k == stop_at:
            out[k] = dict(Huu=Huu)
            break
        sol = solve(Huu, -np.concatenate([Hux, hu[:, None]], axis=1))
        K, kk = sol[:, :22], sol[:, 22]
        s = st["q"] + st["A"].T @ Sb + Hux.T @ kk
        T = st["Q"] + st["A"].T @ SA + Hux.T @ K
        S = (T + T.T) / 2
        out[k] = dict(K=K, k=kk, Huu=Huu, Hux=Hux, hu=hu)
    return out


def _stop(i):
    return FLAG_STAGE if i in FLAG_CASES else None


@functools.lru_cache(None)
def reference():
    """per case: dict(stages={k: K, k, Huu, Hux, hu in longdouble} of the held stages, pivots={k: d})"""
    out = []
    for i, stages in enumerate(_data()):
        rec = recursion(stages, lambda a: a.astype(LD), solve_cholesky_loops, _stop(i))
        piv = {k: _ldl_pivots(v["Huu"]) for k, v in rec.items()}
        out.append(dict(stages={k: v for k, v in rec.items() if "K" in v}, pivots=piv))
    return out


def figures(ref_stage, K, kv):
    """the four figures of one stage: K [nu][22], kv [nu] (any arithmetic) against the reference stage"""
    K, kv = np.asarray(K).astype(LD), np.asarray(kv).astype(LD)
    Kr, kr, Huu, Hux, hu = (ref_stage[key] for key in ("K", "k", "Huu", "Hux", "hu"))
    ninf = lambda m: np.abs(m).sum(axis=1).max() if m.ndim == 2 else np.abs(m).max()   # noqa: E731
    fK = np.abs(K - Kr).max() / max(LD(1), np.abs(Kr).max())
    fk = np.abs(kv - kr).max() / max(LD(1), np.abs(kr).max())
    bK = ninf(Huu @ K + Hux) / (ninf(Huu) * ninf(K) + ninf(Hux))
    bk = ninf(Huu @ kv + hu) / (ninf(Huu) * ninf(kv) + ninf(hu))
    return np.array([float(fK), float(fk), float(bK), float(bk)])


FAMILY = (("LAPACK Cholesky", solve_lapack_cholesky), ("numpy.linalg.solve", solve_lu), ("root-free U D U' loops", solve_udu_loops))


@functools.lru_cache(None)
def family_distances():
    """[case][member][figure]: the worst stage of each plain float64 evaluation of the recursion against the reference"""
    ref = reference()
    out = np.zeros((NCASES, len(FAMILY), 4))
    for i, stages in enumerate(_data()):
        for m, (_, solve) in enumerate(FAMILY):
            rec = recursion(stages, lambda a: a.astype(np.float64), solve, _stop(i))
            for k, r in ref[i]["stages"].items():
                out[i, m] = np.maximum(out[i, m], figures(r, rec[k]["K"], rec[k]["k"]))
    return out


@functools.lru_cache(None)
def bounds():
    """[case][figure]"""
    b = FACTOR * family_distances().max(axis=1) + FLOOR
    b.setflags(write=False)
    return b


# ------------------------------------------------------------------------------------------------------------------ what the code is fed
def arrays(case_ids=tuple(range(NCASES)), shift=()):
    """The arguments of hb_riccati_gains / emu_riccati_gains for the given cases in the given order: (N, n_f, n_z, A, B, b, Q, R, P,
    q, r), every stage array [n][NMAX][...] padded to 12 inputs (R with I, the rest with zeros: what the record's padding is).  For a
    case in `shift` the widths of stage k are those of stage k + 1 (the last keeps its own): what a sweep would see that took the width
    it fetched one stage ahead for the wrong stage."""
    cs = _data()
    n = len(case_ids)
    N = np.array([len(cs[i]) for i in case_ids], dtype=np.int32)
    n_f, n_z = np.zeros((n, NMAX), dtype=np.int32), np.zeros((n, NMAX), dtype=np.int32)
    A, Q = np.zeros((n, NMAX, 22, 22)), np.zeros((n, NMAX, 22, 22))
    Bm, R, P = np.zeros((n, NMAX, 22, 12)), np.zeros((n, NMAX, 12, 12)), np.zeros((n, NMAX, 12, 22))
    b, q, r = np.zeros((n, NMAX, 22)), np.zeros((n, NMAX, 22)), np.zeros((n, NMAX, 12))
    for row, i in enumerate(case_ids):
        for k, st in enumerate(cs[i]):
            nu = st["nu"]
            src = cs[i][min(k + 1, len(cs[i]) - 1)] if i in shift else st
            n_f[row, k], n_z[row, k] = src["n_f"], src["n_z"]
            A[row, k], Q[row, k], b[row, k], q[row, k] = st["A"], st["Q"], st["b"], st["q"]
            Bm[row, k, :, :nu], P[row, k, :nu], r[row, k, :nu] = st["B"], st["P"], st["r"]
            R[row, k] = np.eye(12)
            R[row, k, :nu, :nu] = st["R"]
    return N, n_f, n_z, A, Bm, b, Q, R, P, q, r


# ------------------------------------------------------------------------------------------------------------------ the checks
def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def check(gains_K, gains_k, ric_fail, what):
    """gains_K [12][NMAX][12][22], gains_k [12][NMAX][12], ric_fail [12] of the twelve cases in order.  Prints the worst ratio
    (distance / bound) of every case before it asserts; returns them, [case][figure]."""
    cs, ref, bnd = cases(), reference(), bounds()
    K, kv, fail = np.asarray(gains_K), np.asarray(gains_k), np.asarray(ric_fail)
    assert K.shape == (NCASES, NMAX, 12, 22) and kv.shape == (NCASES, NMAX, 12) and fail.shape == (NCASES,)
    # structure, exact
    for i, stages in enumerate(cs):
        N = len(stages)
        untouched = (_bits(K[i, N:]) == SENTINEL_BITS).all() and (_bits(kv[i, N:]) == SENTINEL_BITS).all()
        assert untouched, f"{what}: sentinel: case {i} has a gain slot behind its horizon (k >= {N}) that was written"
        for k, st in enumerate(stages):
            nu = st["nu"]
            assert (K[i, k, nu:] == 0.0).all() and (kv[i, k, nu:] == 0.0).all(), \
                f"{what}: padded rows: case {i} stage {k}: rows >= {nu} of the gains are not exactly zero"
    want = np.array([1 if i in FLAG_CASES else 0 for i in range(NCASES)])
    assert np.array_equal(fail, want), f"{what}: ric_fail is {fail.tolist()}, expected {want.tolist()}"
    same = np.array_equal(_bits(K[10]), _bits(K[3])) and np.array_equal(_bits(kv[10]), _bits(kv[3]))
    assert same, f"{what}: case 10 differs from case 3, whose copy it is, in {int((_bits(K[10]) != _bits(K[3])).sum())} words of K"
    # forward and backward error, per stage
    ratios = np.zeros((NCASES, 4))
    worst = [None] * NCASES
    for i in range(NCASES):
        for k, r in ref[i]["stages"].items():
            nu = cs[i][k]["nu"]
            got = K[i, k, :nu], kv[i, k, :nu]
            fig = figures(r, *got) if np.isfinite(got[0]).all() and np.isfinite(got[1]).all() else np.full(4, np.inf)
            rt = fig / bnd[i]
            if worst[i] is None or rt.max() > worst[i][0]:
                worst[i] = (rt.max(), k, int(np.argmax(rt)), fig)
            ratios[i] = np.maximum(ratios[i], rt)
    for i in range(NCASES):
        print(f"[rictwin] {what}: case {i:2d}: distance / bound " + "  ".join(f"{FIGURES[f]} {ratios[i, f]:.3g}" for f in range(4)))
    for i in range(NCASES):
        rt, k, f, fig = worst[i]
        assert rt <= 1.0, f"{what}: {FIGURES[f]}: case {i} stage {k}: {fig[f]:.3e} is {rt:.3g} x its bound {bnd[i, f]:.3e}"
    return ratios
