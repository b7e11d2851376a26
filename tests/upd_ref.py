"""One launch of each single-workgroup update kernel of csrc/solvers.hip and csrc/plan_fista.hip -- cgnr_init / cgnr_update (loop and
register forms), cg_start / cg_start_bregman / cg_update, admm_pre / admm_post / admm_zu, fista_init / fista_update (loop and register
forms, phases 1 and 2) -- restated in NumPy in float64 / complex128 (the sums in longdouble) from src/CGNR.jl:108-185,
src/FISTA.jl:110-189, src/ADMM.jl:236-330 and oracle/rls_oracle.py (cg_inplace), with the gates the kernel-level tests hold the device
to.  tests/test_upd_ref.py anchors every restatement to the oracle and plants mistakes; tests/test_gpu_update_edges.py is the device half.

The device's contract, restated as it is: a step length that was formed in double (alpha, beta of CGNR and cg!) is ROUNDED TO FLOAT32
before it multiplies a vector, and so it is here; FISTA's theta, theta_old and the momentum coefficients are Float32 arithmetic, one
rounding per operation, and so they are here (np.float32 scalars): they are compared bit for bit.

Gates (derived as those of tests/pgm_ref.py, whose helpers are reused), u = 2^-24:

  vectors   |got - want| <= gamma_k S + (the forward error of every rounded scalar, times what it multiplies).
            S: the sum of the magnitudes of the terms of the element; k: the roundings on the longest path, no contraction assumed.
            A COMPLEX step length times a complex element costs sqrt 2: with a = (ar, ai), b = (br, bi) the two parts are sums of
            two products, |ar br| + |ai bi| <= |a| |b| and |ar bi| + |ai br| <= |a| |b| (Cauchy-Schwarz), so the modulus of the
            error of a b + c is within gamma_k (sqrt 2 |a| |b| + |c|), k = 4 (products, their sum, the sum with c, and one spare for
            the negation / the order of the two fused steps).
            A scalar s that the device rounds to Float32 from a double that is itself a quotient of double sums: the device's double
            may differ from the float64 value here by the summation order, d = (n + 4) 2^-53 cond (cond = sum |terms| / |sum|), so the
            two roundings may land one Float32 apart: |s_dev - s| <= (2 u + 4 d) |s| =: ds |s|, and ds |s| |operand| joins the gate.
  copies    p = r (cgnr_init), xold = x, z = x (Bregman) and zero fills: bit for bit.
  sums      pgm_ref.sum_gate: held in double, rounded once, judged on the vector that CAME BACK (r, res: gated outputs themselves).
  integers  iteration, done: exact (the tests keep rel_tol 2e-3 relative away from the ratio it is compared with).
"""
import numpy as np

import pgm_ref as P
from pgm_ref import L, U, gam, redot, sum_gate, _mag  # noqa: F401

REG_NONE, REG_L1, REG_L2, REG_L21 = 0, 1, 2, 3
PROJ_NONE, PROJ_REAL, PROJ_POSITIVE = 0, 1, 2
SQRT2 = float(np.sqrt(2.0))
F32 = np.float32
# the N of the device cases: either side of a wave, of 1024 / 2048 / 4096 / 8192 (the dispatch of cgnr_launch_update and
# fista_launch_update), and a ragged ninth pass
LENGTHS = [1, 63, 64, 65, 1023, 1024, 1025, 2048, 2049, 4096, 4097, 8192, 8193, 9001]
SMALL = [1, 63, 65, 1025]          # what the CPU half plants its mistakes at


def hi(v):
    return np.complex128 if np.iscomplexobj(v) else np.float64


def c64(v):
    return np.asarray(v).astype(hi(np.asarray(v)))


def sumsq(v):
    return redot(np.asarray(v), np.asarray(v))


def cdot(a, b):
    """sum conj(a) b in longdouble: (re, im)"""
    a, b = np.asarray(a), np.asarray(b)
    re = redot(a, b)
    im = L(0)
    if np.iscomplexobj(a):
        im = np.sum(a.real.astype(L) * b.imag.astype(L)) - np.sum(a.imag.astype(L) * b.real.astype(L))
    return complex(float(re), float(im))


def round32(z, cplx):
    """a double (pair) rounded to Float32 part by part, as elem<E>::make((float) re, (float) im)"""
    z = complex(z)
    return complex(float(F32(z.real)), float(F32(z.imag))) if cplx else float(F32(z.real))


def d_sum(n, terms, total):
    """relative distance of two double sums of the same n terms in different orders"""
    t = abs(complex(total))
    return (n + 4) * 2.0 ** -53 * (float(terms) / t if t > 0 else 0.0)


# ---- CGNR --------------------------------------------------------------------------------------------------------------------------------
def cgnr_init(r, rel_tol, max_iter, mistake=None):
    """src/CGNR.jl:108-130 after r = A^H b: x = 0, v = 0, p = r, rr = ||r||^2, z0 = ||r||; done() before the first iteration with
    the reference's NaN ratio when r == 0 (NaN <= relTol is false)"""
    r = np.asarray(r)
    rr = float(sumsq(r))
    z0 = float(np.sqrt(L(sumsq(r))))
    with np.errstate(invalid="ignore", divide="ignore"):
        ratio = F32(np.float64(z0) / np.float64(z0))
    out = {"x": np.zeros_like(r), "v": np.zeros_like(r), "p": r.copy(), "rr": rr, "z0": z0, "iteration": 0,
           "done": int(bool(ratio <= F32(rel_tol)) or 0 >= max_iter)}
    if mistake == "z0_is_rr":            # the mistakes tests/test_upd_ref.py plants
        out["z0"] = rr
    elif mistake == "p_zero":
        out["p"] = np.zeros_like(r)
    elif mistake == "done_gt":
        out["done"] = int(bool(ratio <= F32(rel_tol)) or 0 > max_iter)
    return out


def cgnr_update(x, r, p, v, rr, z0, lam, rel_tol, iteration, max_iter, r_dev=None, f32=True, conj=True, drop_reg=False,
                beta_flip=False, done_gt=False, keep_last=False):
    """src/CGNR.jl:153-185 after v = AHA p.  `r_dev`: the r that came back from the device; then the new rr, beta and p are formed
    from it (the kernel forms them from the r it stored).  `f32` = False keeps alpha and beta in double (the float64 oracle's step, for the
    anchor of tests/test_upd_ref.py).  The other keyword switches are the mistakes tests/test_upd_ref.py plants."""
    cplx = np.iscomplexobj(x)
    lam = float(F32(lam))
    x64, r64, p64, v64 = (c64(a) for a in (x, r, p, v))
    zeta = float(rr)
    pv = cdot(p, v) if conj else complex(np.sum(p64 * v64))
    pp = float(sumsq(p)) if lam > 0 else 0.0
    den = pv + (0.0 if drop_reg else lam * pp)
    with np.errstate(all="ignore"):
        alpha = np.complex128(zeta) / np.complex128(den)
    a = round32(alpha, cplx) if f32 else (complex(alpha) if cplx else float(alpha.real))
    xn = x64 + a * p64
    rn = r64 - a * v64
    if lam > 0 and f32:
        lp = (-F32(lam) * np.asarray(p).view(F32)).view(np.asarray(p).dtype)   # scale(-lambda, p): one rounding per part
        rn = rn + c64(lp) * a
    elif lam > 0:
        rn = rn + (-lam * p64) * a
    if keep_last:
        xn[-1], rn[-1] = x64[-1], r64[-1]
    r_used = rn if r_dev is None else c64(r_dev)
    rr_new = float(sumsq(r_used))
    with np.errstate(all="ignore"):
        beta = np.float64(zeta) / np.float64(rr_new) if beta_flip else np.float64(rr_new) / np.float64(zeta)
        ratio = F32(np.sqrt(np.float64(rr_new)) / np.float64(z0))
    bf = float(F32(beta)) if f32 else float(beta)
    pn = bf * p64 + r_used
    if keep_last:
        pn[-1] = p64[-1]
    it = iteration + 1
    hit = (it > max_iter) if done_gt else (it >= max_iter)
    out = {"x": xn, "r": rn, "p": pn, "alpha": complex(alpha), "a": a, "beta": float(beta), "bf": bf, "zeta": zeta, "rr": rr_new,
           "residual": float(np.sqrt(rr_new)), "iteration": it, "done": int(bool(ratio <= F32(rel_tol)) or hit), "ratio": float(ratio)}
    # what the gates need
    n = x64.size
    terms = float(np.sum(_mag(p) * _mag(v))) + lam * pp
    out["ds_alpha"] = 2 * U + 4 * (d_sum(n, terms, den) + d_sum(n, zeta, zeta))
    out["ds_beta"] = 2 * U + 4 * (d_sum(n, rr_new, rr_new) + d_sum(n, zeta, zeta))
    return out


def cgnr_gates(x, r, p, v, lam, w, r_dev):
    """per element bounds of x, r, p for the step `w` = cgnr_update(...) (module docstring)"""
    lam = float(F32(lam))
    ma, bf = abs(complex(w["a"])), abs(w["bf"])
    ap, av = SQRT2 * ma * _mag(p), SQRT2 * ma * _mag(v)
    S_x = ap + _mag(x)
    S_r = _mag(r) + av + lam * ap
    return {"x": gam(4) * S_x + w["ds_alpha"] * ap,
            "r": gam(9 if lam > 0 else 4) * S_r + w["ds_alpha"] * (av + lam * ap),       # two complex fused steps and scale(-lambda, p)
            "p": gam(2) * (bf * _mag(p) + _mag(r_dev)) + w["ds_beta"] * bf * _mag(p)}     # the product, the sum


# ---- cg! ---------------------------------------------------------------------------------------------------------------------------------
def cg_start(x, b, c, rho, reltol, maxiter, fuse=None, drop_rho=False):
    """the entry of oracle cg_inplace with c = AHA x in place: r = b - (c + rho x), u = r, residual, tol, done.  `fuse` = (beta_y, z, u,
    rho_admm): b = beta_y + rho (z - u) formed on the way (two fused-free steps: + rho z, then - rho u) and xold = x"""
    rho32 = float(F32(rho))
    out = {}
    if fuse is not None:
        by, z, uu, ra = fuse
        ra = float(F32(ra))
        b64 = c64(by) + ra * c64(z) - ra * c64(uu)
        out["beta"] = b64
        out["xold"] = np.asarray(x).copy()
    else:
        b64 = c64(b)
    ci = c64(c) + (0.0 if drop_rho else rho32) * c64(x)
    r = b64 - ci
    out.update(r=r, u=r.copy())
    return out


def cg_start_gates(x, b, c, rho, fuse=None):
    rho32 = abs(float(F32(rho)))
    S_c = _mag(c) + rho32 * _mag(x)
    if fuse is not None:
        by, z, uu, ra = fuse
        ra = abs(float(F32(ra)))
        S_b = _mag(by) + ra * (_mag(z) + _mag(uu))
        kb = 4                                       # two products, two sums
    else:
        S_b, kb = _mag(b), 0
    g = {"r": gam(kb + 3) * (S_b + S_c)}             # rho x, c + ., b - .
    g["u"] = g["r"]
    if fuse is not None:
        g["beta"] = gam(kb) * S_b
    return g


def cg_start_record(r_dev, reltol, maxiter, mistake=None):
    """cg_start_scalars from the r that came back: residual = ||r||, tol = max(Float32(reltol) Float32(residual), 0), done"""
    residual = float(sumsq(r_dev)) if mistake == "residual_squared" else float(np.sqrt(L(sumsq(r_dev))))
    tol = max(float(F32(reltol) * F32(residual)), 0.0)
    if mistake == "tol_is_reltol":
        tol = float(F32(reltol))
    return {"residual": residual, "tol": tol, "iteration": 0, "done": int(0 >= maxiter or bool(F32(residual) <= F32(tol)))}


def cg_start_bregman(x, y, cv, beta_y, rho, keep_z=False):
    """src/SplitBregman.jl:257-267 riding on the start of the next inner iteration: beta_y = (beta_y + y) - AHA x, z = x, u = 0,
    beta = beta_y + rho x, xold = x, r = beta - (AHA x + rho x), u_cg = r"""
    rho32 = float(F32(rho))
    by = (c64(beta_y) + c64(y)) - c64(cv)
    by32 = by.astype(np.asarray(x).dtype)            # stored, and used as stored
    bi = c64(by32) + rho32 * c64(x)
    r = c64(bi.astype(np.asarray(x).dtype)) - (c64(cv) + rho32 * c64(x))
    return {"beta_y": by, "z": (np.zeros_like(x) if keep_z else np.asarray(x).copy()), "zu": np.zeros_like(np.asarray(x)), "beta": bi,
            "xold": np.asarray(x).copy(), "r": r, "u": r.copy()}


def cg_start_bregman_gates(x, y, cv, beta_y, rho):
    rho32 = abs(float(F32(rho)))
    S_by = _mag(beta_y) + _mag(y) + _mag(cv)
    S_bi = S_by + rho32 * _mag(x)
    S_r = S_bi + _mag(cv) + rho32 * _mag(x)
    g = {"beta_y": gam(2) * S_by, "beta": gam(4) * S_bi, "r": gam(7) * S_r}
    g["u"] = g["r"]
    return g


def cg_update(x, u, r, cv, residual, rho, tol, iteration, maxiter, r_dev=None, c_dev=None, f32=True, conj=True, drop_rho=False,
              beta_flip=False, done_gt=False, keep_last=False):
    """one iteration of oracle cg_inplace after cv = AHA u: c = cv + rho u, alpha = residual^2 / <u, c>, x += alpha u, r -= alpha c,
    residual = ||r||, done = it >= maxiter || residual <= tol (both Float32), and, unless done, u = r + beta u with
    beta = residual^2 / prev^2.  `c_dev`, `r_dev`: the vectors that came back (alpha is formed from the stored c, beta and u from the
    stored r)"""
    cplx = np.iscomplexobj(x)
    rho32 = float(F32(rho))
    x64, u64, r64 = c64(x), c64(u), c64(r)
    c_new = c64(cv) + (0.0 if drop_rho else rho32) * u64
    c_used = c_new if c_dev is None else c64(c_dev)
    c_arr = c_used.astype(np.asarray(x).dtype) if f32 else c_used
    uc = cdot(u, c_arr) if conj else complex(np.sum(u64 * c_used))
    res2 = float(residual) * float(residual)
    with np.errstate(all="ignore"):
        alpha = np.complex128(res2) / np.complex128(uc)
    a = round32(alpha, cplx) if f32 else (complex(alpha) if cplx else float(alpha.real))
    xn = x64 + a * u64
    rn = r64 - a * c_used
    if keep_last:
        xn[-1], rn[-1] = x64[-1], r64[-1]
    r_used = rn if r_dev is None else c64(r_dev)
    rr = float(sumsq(r_used))
    res_new = float(np.sqrt(L(sumsq(r_used))))
    it = iteration + 1
    TT = F32 if f32 else np.float64
    done = int(((it > maxiter) if done_gt else (it >= maxiter)) or bool(TT(res_new) <= TT(tol)))
    with np.errstate(all="ignore"):
        beta = TT(np.float64(res2) / np.float64(rr)) if beta_flip else TT(np.float64(rr) / np.float64(res2))
    out = {"c": c_new, "x": xn, "r": rn, "alpha": complex(alpha), "a": a, "residual": res_new, "prev": float(residual), "iteration": it,
           "done": done, "bf": float(beta), "u": (u64 if done else r_used + float(beta) * u64)}
    n = x64.size
    d_res2 = 2 * d_sum(n, 1.0, 1.0) + 4 * 2.0 ** -53        # residual^2 from the device's own double ||r||, squared
    out["ds_alpha"] = 2 * U + 4 * (d_sum(n, float(np.sum(_mag(u) * _mag(c_arr))), uc) + d_res2)
    out["ds_beta"] = 2 * U + 4 * (d_sum(n, rr, rr) + d_res2)
    return out


def cg_update_gates(x, u, r, cv, rho, w, r_dev, c_dev):
    rho32 = abs(float(F32(rho)))
    ma, bf = abs(complex(w["a"])), abs(w["bf"])
    au, ac = SQRT2 * ma * _mag(u), SQRT2 * ma * _mag(c_dev)
    g = {"c": gam(2) * (_mag(cv) + rho32 * _mag(u)),
         "x": gam(4) * (au + _mag(x)) + w["ds_alpha"] * au,
         "r": gam(4) * (ac + _mag(r)) + w["ds_alpha"] * ac}
    if not w["done"]:
        g["u"] = gam(2) * (_mag(r_dev) + bf * _mag(u)) + w["ds_beta"] * bf * _mag(u)
    return g


# ---- ADMM --------------------------------------------------------------------------------------------------------------------------------
def admm_pre(beta, beta_y, z, u, x, rho, accumulate, plus_u=False):
    """src/ADMM.jl:236-243: beta = (accumulate ? beta : beta_y) + rho z - rho u; xold = x unless accumulate"""
    rho32 = float(F32(rho))
    base = c64(beta) if accumulate else c64(beta_y)
    out = {"beta": base + rho32 * c64(z) + (rho32 if plus_u else -rho32) * c64(u)}
    if not accumulate:
        out["xold"] = np.asarray(x).copy()
    return out


def admm_pre_gates(beta, beta_y, z, u, rho, accumulate):
    rho32 = abs(float(F32(rho)))
    return {"beta": gam(4) * (_mag(beta if accumulate else beta_y) + rho32 * (_mag(z) + _mag(u)))}


def admm_post(x, xold, z, zold, u, minus_x=False):
    """src/ADMM.jl:265-299 with Phi = I: u += x - z"""
    return {"u": (c64(u) - c64(x) if minus_x else c64(u) + c64(x)) - c64(z)}


def admm_post_gates(x, z, u):
    return {"u": gam(2) * (_mag(u) + _mag(x) + _mag(z))}


def admm_norms(x, xold, z, zold, u_old, u_new, mistake=None):
    """the seven norms from the Float32 vectors as the kernel had them: each difference is ONE Float32 subtraction (exactly reproducible:
    an IEEE operation on stored values), squared and summed in double.  [(want, bound)] for ||x - xold||, ||z - zold||, ||u_new - u||,
    ||x||, ||z||, ||x - z||, ||u_new||"""
    out = []
    pairs = [(x, xold), (z, zold), (u_new, u_old), (x, None), (z, None), (x, z), (u_new, None)]
    if mistake == "u_old_norm":          # ||u|| of the old u; ||x - zold|| for the primal residual
        pairs[6] = (u_old, None)
    elif mistake == "x_minus_zold":
        pairs[5] = (x, zold)
    for a, b in pairs:
        d = np.asarray(a) if b is None else (np.asarray(a).view(F32) - np.asarray(b).view(F32)).view(np.asarray(a).dtype)
        out.append(P.norm_gate(d))
    return out


def admm_zu(x, z_in, u, reg_kind, lam, proj_kind, z_ready=False, z_dev=None, l1=P.prox_l1):
    """src/ADMM.jl:246-267: x = proj(x), z = prox(x + u, lam) (or the TV prox already in z_in), u += x - z.  `z_dev`: the z that came
    back; u is then formed from it (the kernel forms it from the z it stored)"""
    xp = P.project(c64(x), proj_kind)
    z = c64(z_in) if z_ready else P.prox(xp + c64(u), reg_kind, float(F32(lam)), l1)
    z_used = z if z_dev is None else c64(z_dev)
    return {"x": P.project(np.asarray(x), proj_kind), "z": z, "u": (c64(u) + xp) - z_used}


def admm_zu_gates(x, u, reg_kind):
    S = _mag(x) + _mag(u)
    return {"z": gam(1 + P.k_prox(reg_kind, np.iscomplexobj(x))) * S}        # x + u, the prox


def admm_u_gate(x, z_dev, u):
    return {"u": gam(2) * (_mag(u) + _mag(x) + _mag(z_dev))}


def admm_converged(rk, sk, eps_pri, eps_dua, sigma_abs, rel_tol, swap=False, T=F32):
    """src/ADMM.jl:324-330 as the kernel decides it, from the Float32 residuals and limits of the record: rk < sigma_abs + rel_tol eps_pri
    and sk < sigma_abs + rel_tol eps_dua, one rounding per operation.  `swap`: rk held to the dual limit and sk to the primal one"""
    rk, sk, eps_pri, eps_dua, sigma_abs, rel_tol = (T(v) for v in (rk, sk, eps_pri, eps_dua, sigma_abs, rel_tol))
    lim_pri = sigma_abs + rel_tol * eps_pri
    lim_dua = sigma_abs + rel_tol * eps_dua
    return bool((rk < lim_dua and sk < lim_pri) if swap else (rk < lim_pri and sk < lim_dua))


def admm_decision(norms, rho, sigma_abs, rel_tol, iteration, max_iter, swap=False, T=F32):
    """the Float32 record of admm_zu_kernel from the seven Float32 norms, one rounding per operation"""
    dx, dz, du, nx, nz, nxz, nu = (T(v) for v in norms)
    rho, sigma_abs, rel_tol = T(rho), T(sigma_abs), T(rel_tol)
    delta = (dx + dz) + du
    sk = rho * dz
    eps_pri = max(nx, nz)
    rk = nxz
    eps_dua = rho * nu
    conv = admm_converged(rk, sk, eps_pri, eps_dua, sigma_abs, rel_tol, swap, T)
    return {"delta": delta, "sk": sk, "eps_pri": eps_pri, "rk": rk, "eps_dua": eps_dua, "iteration": iteration + 1,
            "done": int(bool(conv) or iteration + 1 >= max_iter)}


# ---- FISTA -------------------------------------------------------------------------------------------------------------------------------
def fista_init(x0, theta, max_iter, mistake=None):
    """src/FISTA.jl:110-129 after x0 = A^H b: x = xold = 0, res = Inf, ||x0||, theta = theta_old, done = 0 >= iterations"""
    x0 = np.asarray(x0)
    res = np.full_like(x0, np.inf)                    # (Inf, 0) for complex data
    out = {"x": np.zeros_like(x0), "xold": np.zeros_like(x0), "res": res, "norm_x0": float(np.sqrt(L(sumsq(x0)))), "theta": F32(theta),
           "theta_old": F32(theta), "iteration": 0, "done": int(0 >= max_iter)}
    if mistake == "norm_squared":        # the mistakes tests/test_upd_ref.py plants
        out["norm_x0"] = float(sumsq(x0))
    elif mistake == "res_zero":
        out["res"] = np.zeros_like(x0)
    elif mistake == "theta_old_one":
        out["theta_old"] = F32(1)
    return out


def theta_next(theta_old, T=F32):
    t = T(theta_old)
    return (T(1) + np.sqrt(T(1) + T(4) * t * t)) / T(2)


def momentum(theta_old, theta, T=F32):
    """the Float32 coefficients of y = c1 xold + c2 x (src/FISTA.jl:147-148 as the kernel forms them)"""
    to, t = T(theta_old), T(theta)
    return (T(1) - to) / t, (to - T(1)) / t + T(1)


def fista_y(xold, xnew, theta_old, theta, T=F32):
    """(y, its bound): y = c1 xold + c2 xnew in float64 from the Float32 coefficients; exact where c1 == 0 and c2 == 1 (theta_old = 1)"""
    c1, c2 = momentum(theta_old, theta, T)
    y = float(c1) * c64(xold) + float(c2) * c64(xnew)
    if c1 == 0 and c2 == 1:
        return y, np.zeros(y.shape)
    return y, gam(2) * (abs(float(c1)) * _mag(xold) + abs(float(c2)) * _mag(xnew))


def prox_l21(v, thr, slices, proj_kind):
    """ProxL21.jl:30-35 as the kernel applies it: groups {g, g + slen, ...}, slen = n / slices; fac = max((gn - thr) / gn, 0), NaN
    kept; then the projection.  (fac, gn) per element are returned for the gate"""
    v = c64(v)
    n = v.size
    slen = n // slices
    out = v.copy()
    fac = np.ones(n)
    gn = np.zeros(n)
    for g in range(slen):
        idx = np.arange(g, n, slen)
        nrm = float(np.sqrt(np.sum(np.abs(v[idx]) ** 2)))
        with np.errstate(all="ignore"):
            q = np.float64(nrm - thr) / np.float64(nrm)
        f = q if q != q else max(q, 0.0)
        out[idx] = f * v[idx]
        fac[idx], gn[idx] = f, nrm
    # (elements past slices * slen belong to the strided groups as well: k runs to n)
    return P.project(out, proj_kind), fac, gn


def fista_update(xold, y, raw, x0, rho, lam, reg_kind, proj_kind, slices, theta, iteration, max_iter, rel_tol, norm_x0, res_dev=None,
                 y_bound=None, phase=0, tv_out=None, res_norm_in=None, T=F32, l1=P.prox_l1, swap_theta=False, done_le=False,
                 keep_last=False, plus_grad=False):
    """src/FISTA.jl:153-189 after raw = AHA y (restart off), and the next extrapolated point.  `res_dev`: the res that came back; the
    gradient step, ||res|| and everything behind them are then formed from it.  phase 1: res, the gradient step (`tv_in`) and ||res||
    only; phase 2: x = proj(tv_out), then theta, done, y with the ||res|| of phase 1.  Returns the gates with the outputs."""
    rho32 = float(T(rho))
    thr = float(T(rho) * T(lam))
    cplx = np.iscomplexobj(x0)
    out, gates = {}, {}
    if y_bound is None:
        y_bound = np.zeros(np.asarray(x0).shape)
    if phase != 2:
        res = c64(raw) - c64(x0)
        r_used = res if res_dev is None else c64(res_dev)
        grad = c64(y) + (rho32 if plus_grad else -rho32) * r_used
        S = _mag(y) + rho32 * _mag(r_used)
        G = gam(2) * S + y_bound                       # rho res, y - .
        out["res"] = res
        gates["res"] = gam(1) * (_mag(raw) + _mag(x0))
        res_norm = float(np.sqrt(L(sumsq(r_used))))
        if phase == 1:
            out["tv_in"], gates["tv_in"] = grad, G
            out["res_norm"] = res_norm
            return out, gates
        if reg_kind == REG_L21:
            xn, fac, gn = prox_l21(grad, thr, slices, proj_kind)
            with np.errstate(all="ignore"):
                ng = int(np.ceil(grad.size / max(grad.size // slices, 1)))
                d_gn = gam(ng + 3)
                # the norm of a group moves by at most the 2-norm of its members' errors (<= sqrt(ng) max): relative to gn
                slen = grad.size // slices
                Gmax = np.zeros(grad.size)
                for g in range(slen):
                    idx = np.arange(g, grad.size, slen)
                    Gmax[idx] = np.sqrt(np.sum(G[idx] ** 2))
                d_fac = np.where(gn > 0, thr / np.maximum(gn, 1e-300) * (d_gn + Gmax / np.maximum(gn, 1e-300)), 0.0) + 3 * U * np.abs(fac)
            gates["x"] = np.abs(fac) * G + _mag(grad) * d_fac + U * np.abs(fac) * _mag(grad)
        else:
            xn = P.project(P.prox(grad, reg_kind, thr, l1), proj_kind)
            gates["x"] = G + gam(P.k_prox(reg_kind, cplx)) * S
    else:
        xn = P.project(c64(tv_out), proj_kind)
        gates["x"] = np.zeros(xn.shape)                # a copy and a projection: nothing rounds
        res_norm = float(res_norm_in)
    if keep_last:
        xn[-1] = c64(xold)[-1]
    theta_old = T(theta)
    th = theta_next(theta_old, T)
    if swap_theta:
        th, theta_old = theta_old, th
    with np.errstate(all="ignore"):
        rel = T(np.float64(res_norm) / np.float64(norm_x0))
    it = iteration + 1
    conv = (rel <= T(rel_tol)) if done_le else (rel < T(rel_tol))
    done = int(bool(conv) or it >= max_iter)
    out.update(x=xn, res_norm=res_norm, rel_res_norm=rel, theta=th, theta_old=theta_old, iteration=it, done=done)
    return out, gates


# ---- a product the test cannot read: AHA v in float64 and the bound of its Float32 evaluation ------------------------------------------------
def product_gate(A, v, extra=16):
    """(AHA v in float64, the bound of |Float32 evaluation - it| per element) for t = A v, w = A^H t summed in ANY order, fused or not:
    a real inner product of n terms is within gamma_n sum |a| |b|; each part of a complex one is a real inner product of 2 n terms, and
    the modulus of the two parts' errors is within sqrt 2 gamma_{2n + 2} sum |a| |b| (the Cauchy-Schwarz step of the module docstring).
    `extra`: the partial sums a product is split into and added up from (row splits, lanes).  The error of t enters w through |A^H|"""
    A64, v64 = c64(A), c64(v)
    m, n = A64.shape
    cplx = np.iscomplexobj(A64)

    def c(k):
        return SQRT2 * gam(2 * (k + extra) + 2) if cplx else gam(k + extra)

    Aa = np.abs(A64)
    t_abs = Aa @ _mag(v)
    e_t = c(n) * t_abs
    t = A64 @ v64
    return A64.conj().T @ t, c(m) * (Aa.T @ (np.abs(t) + e_t)) + Aa.T @ e_t


# ---- the inputs of the cases ---------------------------------------------------------------------------------------------------------------
def problem(dt, n, seed=0, m=8):
    """A (m x n, column-major, entries O(1 / sqrt n) so that AHA p stays O(1)), b, and a Float32 lambda"""
    rng = np.random.default_rng(9000 + 7 * n + seed)
    A = rng.standard_normal((m, n))
    b = rng.standard_normal(m)
    if np.dtype(dt).kind == "c":
        A = (A + 1j * rng.standard_normal((m, n))) / np.sqrt(2.0)
        b = (b + 1j * rng.standard_normal(m)) / np.sqrt(2.0)
    return np.asfortranarray((A / np.sqrt(n)).astype(dt)), b.astype(dt)


def check(held, group, case, got, want, gates, exact=()):
    P.check_vectors(held, group, case, got, want, gates, exact)


def held_cpu(group, case, err, bound):
    """the CPU twin of the device tests' `held`: err <= bound per entry"""
    err, bound = np.asarray(err, dtype=np.float64).ravel(), np.asarray(bound, dtype=np.float64).ravel()
    bad = np.nonzero(~(err <= bound))[0]
    assert bad.size == 0, f"{group} {case}: {bad.size} entries beyond the bound, first {bad[0]}: {err[bad[0]]:.3e} > {bound[bad[0]]:.3e}"
