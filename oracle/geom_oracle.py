"""NumPy restatements of the primitives the geometry stages share (csrc/mm_geom.h), one per definition.

The stage restatements -- verify_numpy, recover_numpy, resect_numpy, _resect_planar, homography_pair, hpose_pair -- live in
their tests/test_*_cpu.py modules and build on these: the integer hash of the sampling, the workgroup's summation order, the
cyclic Jacobi (batched and scalar), the closed-form K^-1, the 24 sums and the triple rule of the reduced DLT one dimension
down, that DLT itself up to h1, h2, h3, and the polar factor.  Every product-sum is parenthesised as the C header states it.
"""
import math

import numpy as np

EPS = 2.220446049250313e-16
M32 = np.uint64(0xFFFFFFFF)
TRIPLES = ((0, 1, 2), (0, 1, 3), (0, 2, 3), (1, 2, 3))


def pcg(v):
    v = np.asarray(v, np.uint64) & M32
    s = (v * np.uint64(747796405) + np.uint64(2891336453)) & M32
    w = (((s >> ((s >> np.uint64(28)) + np.uint64(4))) ^ s) * np.uint64(277803737)) & M32
    return ((w >> np.uint64(22)) ^ w) & M32


def k_inverse(K):
    K = np.asarray(K, float).reshape(3, 3)
    fx, sk, cx, fy, cy = K[0, 0], K[0, 1], K[0, 2], K[1, 1], K[1, 2]
    return np.array([1.0 / fx, -sk / (fx * fy), (sk * cy - cx * fy) / (fx * fy), 1.0 / fy, -cy / fy])


def block_sum(vals):
    """Sum of the rows of vals [n, N] in the workgroup's order: thread t takes rows t, t + 256, ...; xor butterfly over the 64
    lanes of a wave; the four waves in order."""
    vals = np.asarray(vals, float)
    n, N = vals.shape
    chunks = max(1, -(-n // 256))
    pad = np.zeros((chunks * 256, N))
    pad[:n] = vals
    acc = np.zeros((256, N))
    for ch in range(chunks):
        acc = acc + pad[ch * 256:(ch + 1) * 256]
    a = acc.reshape(4, 64, N)
    lane = np.arange(64)
    for off in (32, 16, 8, 4, 2, 1):
        a = a + a[:, lane ^ off]
    return ((a[0, 0] + a[1, 0]) + a[2, 0]) + a[3, 0]


def jacobi(G, N):
    """Cyclic Jacobi on the batch of symmetric matrices G[i][j] (arrays [B]): -> V[i][j]; eigenvalues on G's diagonal."""
    B = G[0][0].shape
    V = [[np.ones(B) if r == c else np.zeros(B) for c in range(N)] for r in range(N)]
    for _ in range(30):
        rotated = False
        for p in range(N - 1):
            for q in range(p + 1, N):
                apq = G[p][q]
                do = (np.abs(apq) > EPS * np.sqrt(np.abs(G[p][p] * G[q][q]))) & (apq != 0.0)
                if not do.any():
                    continue
                rotated = True
                zeta = (G[q][q] - G[p][p]) / (2.0 * apq)
                tn = np.copysign(1.0, zeta) / (np.abs(zeta) + np.sqrt(1.0 + zeta * zeta))
                cs = 1.0 / np.sqrt(1.0 + tn * tn)
                sn = cs * tn
                for k in range(N):
                    akp, akq = G[k][p], G[k][q]
                    G[k][p] = np.where(do, cs * akp - sn * akq, akp)
                    G[k][q] = np.where(do, sn * akp + cs * akq, akq)
                    vkp, vkq = V[k][p], V[k][q]
                    V[k][p] = np.where(do, cs * vkp - sn * vkq, vkp)
                    V[k][q] = np.where(do, sn * vkp + cs * vkq, vkq)
                for k in range(N):
                    apk, aqk = G[p][k], G[q][k]
                    G[p][k] = np.where(do, cs * apk - sn * aqk, apk)
                    G[q][k] = np.where(do, sn * apk + cs * aqk, aqk)
                G[p][q] = np.where(do, 0.0, G[p][q])
                G[q][p] = np.where(do, 0.0, G[q][p])
        if not rotated:
            break
    return V


def jacobi3(G):
    """Cyclic Jacobi of the header: (eigenvalues [3] = the diagonal, V with the eigenvectors in its columns)."""
    G = [[float(G[r][c]) for c in range(3)] for r in range(3)]
    V = [[1.0 if r == c else 0.0 for c in range(3)] for r in range(3)]
    for _ in range(30):
        rotated = False
        for p in range(2):
            for q in range(p + 1, 3):
                apq = G[p][q]
                if abs(apq) > EPS * math.sqrt(abs(G[p][p] * G[q][q])) and apq != 0.0:
                    rotated = True
                    zeta = (G[q][q] - G[p][p]) / (2.0 * apq)
                    tn = math.copysign(1.0, zeta) / (abs(zeta) + math.sqrt(1.0 + zeta * zeta))
                    cs = 1.0 / math.sqrt(1.0 + tn * tn)
                    sn = cs * tn
                    for k in range(3):
                        akp, akq = G[k][p], G[k][q]
                        G[k][p] = cs * akp - sn * akq
                        G[k][q] = sn * akp + cs * akq
                        vkp, vkq = V[k][p], V[k][q]
                        V[k][p] = cs * vkp - sn * vkq
                        V[k][q] = sn * vkp + cs * vkq
                    for k in range(3):
                        apk, aqk = G[p][k], G[q][k]
                        G[p][k] = cs * apk - sn * aqk
                        G[q][k] = sn * apk + cs * aqk
                    G[p][q] = G[q][p] = 0.0
        if not rotated:
            break
    return [G[0][0], G[1][1], G[2][2]], np.array(V)


def polar3(A):
    """mm_polar3 on a 3 x 3 list / array -> (R [3][3], ok)."""
    G = [[(A[0][r] * A[0][c] + A[1][r] * A[1][c]) + A[2][r] * A[2][c] for c in range(3)] for r in range(3)]
    lam, V = jacobi3(G)
    ok = all(np.isfinite(v) and v > 0 for v in lam)
    with np.errstate(all="ignore"):
        dk = [1.0 / np.sqrt(np.float64(v)) for v in lam]
        W = [[((V[i][0] * dk[0]) * V[j][0] + (V[i][1] * dk[1]) * V[j][1]) + (V[i][2] * dk[2]) * V[j][2] for j in range(3)]
             for i in range(3)]
        R = [[(A[r][0] * W[0][c] + A[r][1] * W[1][c]) + A[r][2] * W[2][c] for c in range(3)] for r in range(3)]
    return np.array(R, float), ok


def plane_terms(ma, mb, u, v):
    """The 24 numbers one row adds to (S, Bu, Bv, C) -> [n, 24]."""
    m = [ma, mb, np.ones(len(ma))]
    r2 = u * u + v * v
    out = np.zeros((len(ma), 24))
    k = 0
    for i in range(3):
        for j in range(i, 3):
            w = m[i] * m[j]
            out[:, k], out[:, 6 + k], out[:, 12 + k], out[:, 18 + k] = w, u * w, v * w, r2 * w
            k += 1
    return out


def triple_measure(ai, bi, aj, bj, ak, bk):
    """(|cross|, longest squared side) of the triangle (i, j, k)."""
    pa, pb, qa, qb, ra, rb = aj - ai, bj - bi, ak - ai, bk - bi, ak - aj, bk - bj
    cr = pa * qb - pb * qa
    d0, d1, d2 = pa * pa + pb * pb, qa * qa + qb * qb, ra * ra + rb * rb
    lng = np.where(d0 > d1, d0, d1)
    lng = np.where(lng > d2, lng, d2)
    return np.abs(cr), lng


def plane_dlt(acc):
    """The reduced DLT of a plane-to-image map on a batch of sums acc [B, 24]: Cholesky of S, h3 by the 3 x 3 Jacobi, h1 and
    h2 by back substitution -> (h1, h2, h3 (lists of three arrays [B]), the pivot verdict [B])."""
    acc = np.asarray(acc, float)
    B = acc.shape[0]
    S, Bu, Bv, M = ([[None] * 3 for _ in range(3)] for _ in range(4))
    k = 0
    for i in range(3):
        for j in range(i, 3):
            S[i][j] = S[j][i] = acc[:, k]
            Bu[i][j] = Bu[j][i] = acc[:, 6 + k]
            Bv[i][j] = Bv[j][i] = acc[:, 12 + k]
            M[i][j] = M[j][i] = acc[:, 18 + k]
            k += 1
    ok = np.ones(B, bool)
    with np.errstate(all="ignore"):
        L = [[None] * 3 for _ in range(3)]
        for j in range(3):
            d = S[j][j]
            for k in range(j):
                d = d - L[j][k] * L[j][k]
            ok &= np.isfinite(d) & (d > 1e-12 * S[j][j])
            ljj = np.sqrt(d)
            L[j][j] = ljj
            for i in range(j + 1, 3):
                v = S[i][j]
                for k in range(j):
                    v = v - L[i][k] * L[j][k]
                L[i][j] = v / ljj
        Yu, Yv = [[None] * 3 for _ in range(3)], [[None] * 3 for _ in range(3)]
        for i in range(3):
            for cc in range(3):
                vu, vv = Bu[i][cc], Bv[i][cc]
                for k in range(i):
                    vu = vu - L[i][k] * Yu[k][cc]
                    vv = vv - L[i][k] * Yv[k][cc]
                Yu[i][cc] = vu / L[i][i]
                Yv[i][cc] = vv / L[i][i]
        for i in range(3):
            for j in range(i, 3):
                tu = (Yu[0][i] * Yu[0][j] + Yu[1][i] * Yu[1][j]) + Yu[2][i] * Yu[2][j]
                tv = (Yv[0][i] * Yv[0][j] + Yv[1][i] * Yv[1][j]) + Yv[2][i] * Yv[2][j]
                M[i][j] = M[j][i] = (M[i][j] - tu) - tv
        V3 = jacobi(M, 3)
        ev = M[0][0]
        h3 = [V3[r][0] for r in range(3)]
        for cc in range(1, 3):
            lower = M[cc][cc] < ev
            ev = np.where(lower, M[cc][cc], ev)
            h3 = [np.where(lower, V3[r][cc], h3[r]) for r in range(3)]
        wu = [(Yu[i][0] * h3[0] + Yu[i][1] * h3[1]) + Yu[i][2] * h3[2] for i in range(3)]
        wv = [(Yv[i][0] * h3[0] + Yv[i][1] * h3[1]) + Yv[i][2] * h3[2] for i in range(3)]
        h1, h2 = [None] * 3, [None] * 3
        for i in (2, 1, 0):
            vu, vv = wu[i], wv[i]
            for k in range(i + 1, 3):
                vu = vu - L[k][i] * h1[k]
                vv = vv - L[k][i] * h2[k]
            h1[i] = vu / L[i][i]
            h2[i] = vv / L[i][i]
    return h1, h2, h3, ok


def factor_from(x, tol):
    """How many times x is away from tol, in either direction (inf for x = 0 against a positive tol)."""
    if x == tol:
        return 1.0
    if x == 0.0 or tol == 0.0:
        return math.inf
    return max(x / tol, tol / x)
