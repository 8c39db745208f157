"""fp64 restatement of the spectral-normalisation kernels (csrc/specnorm.hip) with per-element error bounds derived from the
kernels' summation shape, as tests/norm_ref.py does for the normalisation passes. tests/test_sn_ref_cpu.py proves the
restatement against torch.nn.utils.spectral_norm; the GPU tests hold the kernels against it.

Semantics (torch.nn.utils.spectral_norm, eps = 1e-12), W a ca x K matrix in torch's column order (weight.view(ca, -1)):
  train:  `iters` times  v = W^T u / max(|W^T u|, eps),  u = W v / max(|W v|, eps);   sigma = u . (W v);   W_sn = W / sigma
  eval:   sigma from the stored u, v
  backward (u, v constants, sigma differentiated through W):  dL/dW = (G - <G, W_sn>_F u v^T) / sigma,  G = dL/dW_sn

Error model. One fp32 operation rounds by at most U = 2^-24 relative; a sum whose longest chain of dependent roundings is k deep
errs by at most gamma(k) = k U / (1 - k U) times the sum of the magnitudes of its terms, whatever the order. The depths are read
off the kernels:
  W^T u   per column: a chain of min(ca, 16) fused multiply-adds per 16-row chunk, then the chunks added in order
  |t|^2   per 256-column tile: the square, a 6-level wave tree, 3 adds over the waves; then the tiles added in order; one sqrt
  W v     per row: per lane at most 16 fused multiply-adds (1024-column chunk / 64 lanes), the wave tree, then the chunks in order
  |s|^2, u . s   per thread ceil(ca / 256) fused multiply-adds, the wave tree, 3 adds
  <G, W>  per thread 16 fused multiply-adds, wave tree, 3 adds per 4096-element chunk; the chunks: ceil(chunks / 256) adds per
          thread, wave tree, 3 adds
Input errors are carried from stage to stage to first order with the exact denominators kept (no hidden constant)."""
import numpy as np

U = 2.0 ** -24
EPS = 1e-12
ROWS, CTILE, CCHUNK, DCHUNK = 16, 256, 1024, 4096


def gamma(k):
    return k * U / (1.0 - k * U)


def col_map(K, cb):
    """j[m]: column of torch's weight.view(ca, -1) held by memory column m of the master layout [a][ky][kx][b] (cb = 0: identity)."""
    m = np.arange(K)
    return m if cb == 0 else (m % cb) * 16 + m // cb


def to_torch_order(w_mem, cb):
    """ca x K matrix in memory column order -> torch's column order."""
    out = np.empty_like(w_mem)
    out[:, col_map(w_mem.shape[1], cb)] = w_mem
    return out


def to_memory_order(w_torch, cb):
    return w_torch[:, col_map(w_torch.shape[1], cb)]


def power_iteration(W, u, v, iters, train):
    """fp64. -> (u, v, sigma)"""
    W, u, v = np.asarray(W, np.float64), np.asarray(u, np.float64).copy(), np.asarray(v, np.float64).copy()
    if train:
        for _ in range(iters):
            t = W.T @ u
            v = t / max(np.linalg.norm(t), EPS)
            s = W @ v
            u = s / max(np.linalg.norm(s), EPS)
    return u, v, float(u @ (W @ v))


def project(G, W_sn, u, v, sigma):
    """dL/dW from G = dL/dW_sn (fp64)."""
    G = np.asarray(G, np.float64)
    c = float((G * np.asarray(W_sn, np.float64)).sum())
    return (G - c * np.outer(u, v)) / sigma


def _normalise_bound(t, e_t, E_t, depth_sq):
    """x = t / |t| computed from t_hat, |t_hat - t| <= e_t per element and <= E_t in the 2-norm: -> (per-element bound on
    |x_hat - x|, 2-norm bound)."""
    n = np.linalg.norm(t)
    d = max(n, EPS)
    rel = gamma(depth_sq + 2) + E_t / d          # |d_hat - d| <= rel d: the sum of squares, the sqrt, the inputs
    assert rel < 0.5, "the bound's first-order model needs a well-conditioned norm"
    den = d * (1 - rel)
    e_x = (e_t + np.abs(t) * rel / (1 - rel)) / den + U * (np.abs(t) + e_t) / den
    E_x = (E_t + n * rel / (1 - rel)) / den + U * (n + E_t) / den
    return e_x, E_x


def _matvec_bound(M, aM, x, e_x, E_x, depth, nM, naM):
    """y = M x computed in fp32 from x_hat: rounding gamma(depth) |M| |x_hat| per element; the input error passes through M
    itself, bounded in the 2-norm by |M|_2 E_x (an element of a vector is at most its 2-norm). -> (per element, 2-norm)"""
    r = gamma(depth) * (aM @ np.abs(x))
    prop = (gamma(depth) * naM + nM) * E_x
    return np.minimum(r + prop, r + gamma(depth) * (aM @ e_x) + aM @ e_x), np.linalg.norm(r) + prop


def power_iteration_bounds(W, u, v, iters, train):
    """-> dict(u, v, sigma: fp64 reference; eu, ev, esigma: bounds on what specnorm.hip may return). W, u, v: fp32 values."""
    W = np.asarray(W, np.float64)
    ca, K = W.shape
    aW = np.abs(W)
    nW, naW = np.linalg.norm(W, 2), np.linalg.norm(aW, 2)
    rch, ct, cch = -(-ca // ROWS), -(-K // CTILE), -(-K // CCHUNK)
    d_t = min(ca, ROWS) + rch
    d_s = min(16, -(-K // 64)) + 6 + cch
    d_q = -(-ca // 256) + 9
    u = np.asarray(u, np.float64).copy()
    v = np.asarray(v, np.float64).copy()
    eu, ev, Eu, Ev = np.zeros(ca), np.zeros(K), 0.0, 0.0
    for _ in range(iters if train else 0):
        t = W.T @ u
        e_t, E_t = _matvec_bound(W.T, aW.T, u, eu, Eu, d_t, nW, naW)
        ev, Ev = _normalise_bound(t, e_t, E_t, 10 + ct)
        v = t / max(np.linalg.norm(t), EPS)
        s = W @ v
        e_s, E_s = _matvec_bound(W, aW, v, ev, Ev, d_s, nW, naW)
        eu, Eu = _normalise_bound(s, e_s, E_s, d_q)
        u = s / max(np.linalg.norm(s), EPS)
    s = W @ v
    e_s, E_s = _matvec_bound(W, aW, v, ev, Ev, d_s, nW, naW)
    sigma = float(u @ s)
    ns, nu = np.linalg.norm(s), np.linalg.norm(u)
    # u_hat . s_hat - u . s = rounding + (u_hat - u) . s_hat + u . (s_hat - s), the inner products by Cauchy-Schwarz
    esigma = float(gamma(d_q) * ((np.abs(u) + eu) @ (np.abs(s) + e_s)) + Eu * (ns + E_s) + nu * E_s)
    return {"u": u, "v": v, "sigma": sigma, "eu": eu, "ev": ev, "esigma": esigma}


def effective_bound(W, sigma, esigma):
    """|W / sigma_hat - W / sigma| per element, plus the division's rounding."""
    aW = np.abs(np.asarray(W, np.float64))
    lo = abs(sigma) - esigma
    assert lo > 0
    return aW * esigma / (abs(sigma) * lo) + U * aW / lo


def dot_depth(n):
    """Longest chain of roundings in <G, W_eff> over n elements (module docstring)."""
    dch = -(-n // DCHUNK)
    return min(16, -(-n // 256)) + 9 + -(-dch // 256) + 9


def project_bounds(G, W_sn, u, v, sigma, scale, dst0):
    """-> (reference of dst0 + scale * project(...), per-element bound). All inputs fp32 values, taken as exact."""
    G, W_sn = np.asarray(G, np.float64), np.asarray(W_sn, np.float64)
    u, v = np.asarray(u, np.float64), np.asarray(v, np.float64)
    d_c = dot_depth(G.size)
    c = float((G * W_sn).sum())
    e_c = gamma(d_c) * float((np.abs(G) * np.abs(W_sn)).sum())
    uv = np.abs(np.outer(u, v))
    add = scale * (G - c * np.outer(u, v)) / sigma
    ref = np.asarray(dst0, np.float64) + add
    # c u, (c u) v, the subtraction, the division, the scale, the accumulation: one rounding each
    bound = abs(scale) / abs(sigma) * (e_c * uv + 5 * U * (np.abs(G) + (abs(c) + e_c) * uv)) + U * (np.abs(ref) + np.abs(add))
    return ref, bound


def critic_matrices(P):
    """{layer prefix: (ca x K fp32 matrix in torch's column order)} of a PatchGAN parameter dict with logical shapes."""
    out = {}
    for idx in (0, 2, 5, 8, 11, 13):
        for leaf in ("weight_orig", "weight"):
            k = f"model.{idx}.{leaf}"
            if k in P:
                w = np.asarray(P[k], np.float32)
                out[f"model.{idx}"] = w.reshape(w.shape[0], -1)
    return out
