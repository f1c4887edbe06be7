"""The reference of -a=tvl1 with the illumination channel (dfx_params.tvl1_gamma): a three-channel NumPy restatement
assembled from the pieces of tests/numpy_restatement.py (imported, not edited; oracle/ has no gamma and stays as it is).

Test infrastructure only.  Semantics (SURVEY.md Appendix A "with gamma"; restated from memory of opencv_contrib 4.5.x,
rated MED, parity unpinned): beside u1, u2 every level has a plane u3, zero at the coarsest level and carried down by the
same bilinear resize WITHOUT the 1/scaleStep factor; p31 = p32 = 0 once per level; the warp is unchanged;
    rho   = rho_c + ((I1wx*u1 + I1wy*u2) + gamma*u3)          (gamma as float)
    d3    = l_t*gamma | -l_t*gamma | fi*gamma | 0             (the three thresholding branches and the fourth case)
    u3new = (u3 + d3) + theta*div(p31, p32)
    diff  = (u1-u1new)^2 + (u2-u2new)^2                        (u3 does not enter the convergence sum)
and (p31, p32) take the dual update of (p11, p12) on u3's clamped forward differences.  With gamma = 0 this is
oracle.tvl1_calc bit for bit and u3 stays 0 (tests/test_tvl1_gamma_ref.py)."""
from __future__ import annotations

import numpy as np

from tests.numpy_restatement import centered_gradient, cv_round, divergence, hypot_cuda, resize_linear, warp_backward

F = np.float32


def _estimate_u(I1wx, I1wy, grad, rho_c, p, u, l_t, theta, gamma, calc_error):
    """A.6 with gamma.  p = [(p11, p12), (p21, p22), (p31, p32)], u = [u1, u2, u3]; returns the new u and sum(diff)."""
    rho = rho_c + ((I1wx * u[0] + I1wy * u[1]) + gamma * u[2])
    lg = l_t * grad
    c1 = rho < -lg
    c2 = (~c1) & (rho > lg)
    c3 = (~c1) & (~c2) & (grad > np.finfo(F).eps)
    with np.errstate(divide="ignore", invalid="ignore"):
        fi = np.where(c3, -rho / np.where(c3, grad, F(1)), F(0)).astype(F)
    new = []
    for ch, wgt in enumerate((I1wx, I1wy, gamma)):
        d = np.where(c1, l_t * wgt, np.where(c2, -(l_t * wgt), np.where(c3, fi * wgt, F(0)))).astype(F)
        v = u[ch] + d
        new.append((v + theta * divergence(p[ch][0], p[ch][1])).astype(F))
    err = 0.0
    if calc_error:
        e1, e2 = u[0] - new[0], u[1] - new[1]
        err = float((e1 * e1 + e2 * e2).astype(F).astype(np.float64).sum())
    return new, err


def _estimate_dual(u, pa, pb, taut):
    """A.7 for one channel: forward differences with clamp, hypot as CUDA evaluates it, IEEE division."""
    ux = np.zeros_like(u)
    uy = np.zeros_like(u)
    ux[:, :-1] = u[:, 1:] - u[:, :-1]
    uy[:-1, :] = u[1:, :] - u[:-1, :]
    ng = F(1) + taut * hypot_cuda(ux, uy)
    return ((pa + taut * ux) / ng).astype(F), ((pb + taut * uy) / ng).astype(F)


def _proc_one_scale(I0, I1, u, gamma, warps, iterations, epsilon, lam, theta, tau):
    h, w = I0.shape
    thr = epsilon * epsilon * float(w * h)
    l_t, taut, theta = F(lam * theta), F(tau / theta), F(theta)
    I1x, I1y = centered_gradient(I1)
    p = [(np.zeros((h, w), F), np.zeros((h, w), F)) for _ in range(3)]
    iters, checks = [], 0
    for _ in range(warps):
        I1wx, I1wy, grad, rho_c = warp_backward(I0, I1, I1x, I1y, u[0], u[1])
        error = np.finfo(np.float64).max
        prev = 0.0
        n = 0
        while error > thr and n < iterations:
            calc = (epsilon > 0) and bool(n & 1) and (prev < thr)
            u, e = _estimate_u(I1wx, I1wy, grad, rho_c, p, u, l_t, theta, gamma, calc)
            if calc:
                error = prev = e
                checks += 1
            else:
                error = np.finfo(np.float64).max
                prev -= thr
            p = [_estimate_dual(u[ch], p[ch][0], p[ch][1], taut) for ch in range(3)]
            n += 1
        iters.append(n)
    return u, iters, checks


def tvl1_gamma_calc(frame0, frame1, gamma, nscales=5, warps=5, iterations=300, epsilon=0.01, scale_step=0.8, tau=0.25,
                    lam=0.15, theta=0.3):
    """Returns (flow (H, W, 2), u3 at level 0, iteration table [level][warp], convergence sums evaluated)."""
    gamma = F(gamma)
    I0s, I1s = [frame0.astype(F)], [frame1.astype(F)]
    ifs = F(1.0 / scale_step)
    n = nscales
    for s in range(1, nscales):
        ph, pw = I0s[-1].shape
        w, h = cv_round(pw * scale_step), cv_round(ph * scale_step)
        if w < 16 or h < 16:
            n = s
            break
        I0s.append(resize_linear(I0s[-1], w, h, ifs, ifs))
        I1s.append(resize_linear(I1s[-1], w, h, ifs, ifs))
    u = [np.zeros(I0s[n - 1].shape, F) for _ in range(3)]
    table, checks = [None] * n, 0
    for s in range(n - 1, -1, -1):
        u, table[s], ck = _proc_one_scale(I0s[s], I1s[s], u, gamma, warps, iterations, epsilon, lam, theta, tau)
        checks += ck
        if s > 0:
            dh, dw = I0s[s - 1].shape
            sh, sw = I0s[s].shape
            ifx, ify = F(1.0 / (dw / sw)), F(1.0 / (dh / sh))
            up = [F(1.0 / scale_step), F(1.0 / scale_step), None]  # u3: the same resize, no factor
            u = [resize_linear(u[ch], dw, dh, ifx, ify) for ch in range(3)]
            u = [(u[ch] * up[ch]).astype(F) if up[ch] is not None else u[ch] for ch in range(3)]
    return np.stack([u[0], u[1]], axis=-1), u[2], table, checks
