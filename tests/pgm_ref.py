"""One update of OptISTA and of POGM -- everything of `iterate` behind res = AHA x -- restated in NumPy from the reference
(src/OptISTA.jl:176-204, src/POGM.jl:176-233) and from oracle/rls_oracle.py, with the scalars the C ABI takes
(rls_optista_update, rls_pogm_update, rls_pogm_update_auto): the checker of the fused kernels of csrc/pgm.hip.

Every step runs at `prec` = float64 (complex128 for complex data; the sums in longdouble) or, from the same lines, at float32
(complex64) with one rounding per operation: no operation is fused, a real scalar times a complex vector rounds each part once.
The coefficients are Float32 numbers in either case (the host forms them in Float32, as the reference's Float32 path does), and
the L1 prox carries eps(Float32) in either case: the float64 run is the exact value of the Float32 operation, not another
operation.

The gates of the kernel-level tests are here too (tests/test_pgm_ref.py holds the CPU half, tests/test_gpu_pgm_edges.py the device
half), so that both halves use the same numbers.  With u = 2^-24:

  vectors   |got - want| <= gamma_k S, gamma_k = k u / (1 - k u).  S: the sum of the magnitudes of the output's terms,
            sum |coef| |operand|, where an operand that is itself a computed value enters with ITS S (the prox and the
            projections are non-expansive: their output enters with the S of their input).  k: the roundings on the longest
            path from the inputs to the output, counted without any contraction (a fused multiply-add only removes one):
              - the products of one sum count once together (their errors add up to u sum |term| <= u S), every addition once
                (u |partial sum| <= u S);
              - an operand that is a computed value brings its own k along: its error, times the coefficient, is
                k' u |coef| S' <= k' u S.
            Complex data: every operation here is a real scalar times, or a sum of, complex numbers, i.e. the same real
            operation on both parts; with S_re, S_im the part-wise sums, sqrt(S_re^2 + S_im^2) <= S (Minkowski), so the
            modulus of the error obeys the same k and no sqrt 2 is needed even where the compiler contracts the two parts
            differently.
            prox L1 (ProxL1.jl:18-22), out = sh (v + eps) / (a + eps), a = |v|, sh = max(a - thr, 0) <= a:
              complex  a = hypot: 1 ulp = 2 u;  sh: 2 u a + u sh;  v.re + eps, the product, a + eps (2 u + u), the quotient:
                       6 u on a value of magnitude sh  ->  (2 a + sh) u + 6 sh u <= 9 u a:                             k_prox = 9
              real     a is exact:  sh, v + eps, product, a + eps, quotient: 5 u sh:                                   k_prox = 5
            prox L2 (ProxL2.jl:18-21): the factor and the product in double, one rounding on store:                    k_prox = 1
            (REG_NONE: 0; the projections round nothing)
  copies    zold, xold: bit for bit.
  sums      held in double, rounded once: |got - want| <= u |want| + (n + 4) 2^-53 sum |terms|, where `want` is the longdouble sum
            of the terms AS THE DEVICE HAD THEM: ||res|| from the res vector that came back (a gated output itself).  The first
            factor of POGM's three dot products, w + y + rho / gamma (x - z) (:223), is never stored; it is formed in float64
            from w and the x1, x, z that came back, which leaves its own four roundings (the two products together, three
            additions), so these three gates carry sum_i 4 u S_w'[i] |second factor[i]| on top.
"""
import math

import numpy as np

REG_NONE, REG_L1, REG_L2 = 0, 1, 2
PROJ_NONE, PROJ_REAL, PROJ_POSITIVE = 0, 1, 2
U = 2.0 ** -24
EPS32 = 2.0 ** -23          # eps(Float32)
L = np.longdouble


def _elem_type(v, prec):
    T = np.dtype(prec).type
    return T, (np.result_type(T, np.complex64).type if np.iscomplexobj(v) else T)


def _cast(v, prec):
    _, E = _elem_type(v, prec)
    return np.array(v, dtype=E, order="C")


def _scale(s, v):
    """real scalar times vector: one rounding per part"""
    T = v.real.dtype.type
    return (T(s) * v.view(T)).view(v.dtype)


def redot(a, b):
    """sum of real(conj(a) b), exact products, longdouble sum"""
    s = np.sum(a.real.astype(L) * b.real.astype(L))
    if np.iscomplexobj(a):
        s += np.sum(a.imag.astype(L) * b.imag.astype(L))
    return s


def _scalar(s, prec):
    return np.dtype(prec).type(s)


# ---- prox / projection ---------------------------------------------------------------------------------------------------------------
def prox_l1(v, thr, eps_imag=False, eps=EPS32):
    """ProxL1.jl:18-22: x = max(|x| - thr, 0) (x + eps) / (|x| + eps), eps = eps(Float32) added to the real part only.
    `eps_imag`: the mistake of adding it to the imaginary part too (tests/test_pgm_ref.py plants it); `eps`: another type's eps
    (the float64 oracle's, where the step is compared with it)"""
    T = v.real.dtype.type
    a = np.abs(v)
    sh = np.maximum(a - T(thr), T(0))
    den = a + T(eps)
    re = (sh * (v.real + T(eps))) / den
    if not np.iscomplexobj(v):
        return re
    im = v.imag + T(eps) if eps_imag else v.imag
    out = np.empty_like(v)
    out.real = re
    out.imag = (sh * im) / den
    return out


def prox_l2(v, thr):
    """ProxL2.jl:18-21: the Float64 literals make the factor a double; the product is rounded on store"""
    f = 1.0 / (1.0 + 2.0 * float(thr))
    hi = np.complex128 if np.iscomplexobj(v) else np.float64
    return (v.astype(hi) * f).astype(v.dtype)


def prox(v, reg_kind, thr, l1=prox_l1):
    if reg_kind == REG_L1:
        return l1(v, thr)
    if reg_kind == REG_L2:
        return prox_l2(v, thr)
    assert reg_kind == REG_NONE, reg_kind
    return v.copy()


def project(v, proj_kind):
    """ProxReal.jl:16-19 (the imaginary part dropped), ProxPositive.jl:16-20 (real, then negative real parts to zero)"""
    assert proj_kind in (PROJ_NONE, PROJ_REAL, PROJ_POSITIVE), proj_kind
    out = v.copy()
    if proj_kind == PROJ_NONE:
        return out
    if np.iscomplexobj(out):
        out.imag = 0
    if proj_kind == PROJ_POSITIVE:
        re = out.real if np.iscomplexobj(out) else out
        re[re < 0] = 0
    return out


# ---- the steps -----------------------------------------------------------------------------------------------------------------------
def optista_step(res, x0, x, y, z, step, reg_kind, thr, c_z, c_y, c_x, c_zn, c_zo, prec=np.float64, l1=prox_l1):
    """src/OptISTA.jl:180-199 with step = rho gamma, thr = rho gamma lambda, c_z = -1 / gamma, c_y = 1 / gamma, c_x = -beta,
    c_zn = 1 + alpha + beta, c_zo = -alpha.  `res` holds AHA x on entry."""
    res, x0, x, y, z = (_cast(v, prec) for v in (res, x0, x, y, z))
    zold = z.copy()                                 # :180  zold .= z
    yold = y.copy()                                 # :181  z .= y
    r = res - x0                                    # :183
    yn = y - _scale(step, r)                        # :184
    yn = prox(yn, reg_kind, thr, l1)                # :190
    zn = _scale(c_z, yold)                          # :195  z ./= -gamma
    zn = zn + (x + _scale(c_y, yn))                 # :196  z .+= x .+ y ./ gamma
    xn = _scale(c_x, x)                             # :197
    xn = xn + _scale(c_zn, zn)                      # :198
    xn = xn + _scale(c_zo, zold)                    # :199  x .-= alpha .* zold
    return {"res": r, "x": xn, "y": yn, "z": zn, "zold": zold, "res_norm": _scalar(np.sqrt(redot(r, r)), prec)}


def pogm_step(res, x0, xbuf, ybuf, z, w, rho, c_y, c_x1, c_xo, c_z, reg_kind, thr, proj_kind, restart, rg, prec=np.float64,
              l1=prox_l1, rg_flip=False):
    """src/POGM.jl:180-231 with c_y = -alpha, c_x1 = 1 + alpha + beta, c_xo = -(beta + rho alpha / gamma_old),
    c_z = rho alpha / gamma_old, thr = gamma lambda, rg = rho / gamma.  xbuf holds x_k and ybuf y_{k-1} on entry; on exit xbuf
    holds the gradient point (the reference's y after its swap, :206-208) and ybuf the new x.  `rg_flip`: the mistake of
    applying rg to z with the wrong sign in :223 (tests/test_pgm_ref.py plants it)"""
    res, x0, xbuf, ybuf, z = (_cast(v, prec) for v in (res, x0, xbuf, ybuf, z))
    xold = xbuf.copy()                              # :180
    r = res - x0                                    # :182
    x1 = xbuf - _scale(rho, r)                      # :183
    xn = _scale(c_y, ybuf)                          # :209  (x and y swapped: x is y_{k-1} now)
    xn = xn + _scale(c_x1, x1)                      # :210
    xn = xn + _scale(c_xo, xold)                    # :211
    xn = xn + _scale(c_z, z)                        # :212
    zn = xn.copy()                                  # :213
    xn = project(prox(xn, reg_kind, thr, l1), proj_kind)   # :216-219
    out = {"res": r, "xbuf": x1, "ybuf": xn, "xold": xold, "z": zn, "res_norm": _scalar(np.sqrt(redot(r, r)), prec)}
    if restart:
        w = _cast(w, prec)
        wi = w + (x1 + _scale(rg, (xn + zn) if rg_flip else (xn - zn)))   # :223
        out.update(dwx=_scalar(redot(wi, xn), prec), dwz=_scalar(redot(wi, zn), prec), dwr=_scalar(redot(wi, r), prec))
        out["w"] = _scale(rg, zn - xn) - x1         # :231
    else:
        out.update(dwx=None, dwz=None, dwr=None, w=None if w is None else _cast(w, prec))
    return out


# ---- the scalar recurrences, in the reference's operation order at type T ----------------------------------------------------------------
def theta_next(th, last, T=np.float32):
    """:171 / :173 (OptISTA), :191 / :193 (POGM)"""
    th = T(th)
    return (T(1) + np.sqrt(T(1) + T(8 if last else 4) * th * th)) / T(2)


def optista_coefs(theta, theta_n, last, rho, lam, T=np.float32):
    """src/OptISTA.jl:168-176 and the scalars of :184-199: the float arguments of rls_optista_update, and the new theta"""
    th, tn, rho = T(theta), T(theta_n), T(rho)
    gamma = T(2) * th / (tn * tn) * (tn * tn - T(2) * th * th + th)
    thn = theta_next(th, last, T)
    alpha, beta = (th - T(1)) / thn, th / thn
    return {"theta": thn, "gamma": gamma, "step": rho * gamma, "thr": rho * gamma * T(lam), "c_z": T(-1) / gamma, "c_y": T(1) / gamma,
            "c_x": -beta, "c_zn": T(1) + alpha + beta, "c_zo": -alpha}


def pogm_coefs(theta, sigma, gamma_old, last, rho, lam, restart, T=np.float32):
    """src/POGM.jl:189-202 and the scalars of :209-231: the float arguments of rls_pogm_update, the new theta and gamma"""
    tho, sigma, gamma_old, rho = T(theta), T(sigma), T(gamma_old), T(rho)
    thn = theta_next(tho, last and restart, T)
    alpha = (tho - T(1)) / thn
    beta = sigma * tho / thn
    c_x1 = T(1) + alpha + beta
    gamma = rho * c_x1 if restart else rho * (T(2) * tho + thn - T(1)) / thn
    c_z = rho * alpha / gamma_old
    return {"theta": thn, "alpha": alpha, "beta": beta, "gamma": gamma, "rho": rho, "c_y": -alpha, "c_x1": c_x1,
            "c_xo": -(beta + c_z), "c_z": c_z, "thr": gamma * T(lam), "rg": rho / gamma}


def pogm_auto_coefs(theta, sigma, gamma_old, last, rho, lam, T=np.float32):
    """restart = :gradient: what rls_pogm_update_auto forms on the device from its record"""
    return pogm_coefs(theta, sigma, gamma_old, last, rho, lam, True, T)


def pogm_restart(gamma, dwx, dwz, dwr, T=np.float32):
    """:224  real((w . x - w . z) / gamma - w . res) < 0, from the three real parts"""
    crit = (T(dwx) - T(dwz)) / T(gamma) - T(dwr)
    return bool(crit < 0), crit


def pogm_auto_record(theta_old, sigma, sigma_fac, coefs, restart, T=np.float32):
    """(theta, theta_old, sigma, gamma) after the iteration (:189, :225-230)"""
    if restart:
        return T(1), T(theta_old), T(1), coefs["gamma"]
    return coefs["theta"], T(theta_old), T(sigma) * T(sigma_fac), coefs["gamma"]


# ---- the gates -----------------------------------------------------------------------------------------------------------------------
def gam(k):
    return k * U / (1.0 - k * U)


def k_prox(reg_kind, cplx):
    return {REG_NONE: 0, REG_L1: 9 if cplx else 5, REG_L2: 1}[reg_kind]


def _mag(v):
    return np.abs(np.asarray(v).astype(np.complex128))


def optista_gates(res, x0, x, y, z, step, reg_kind, thr, c_z, c_y, c_x, c_zn, c_zo):
    """per element bounds of res, y, z, x (module docstring)"""
    kp = k_prox(reg_kind, np.iscomplexobj(x))
    step, c_z, c_y, c_x, c_zn, c_zo = (abs(float(c)) for c in (step, c_z, c_y, c_x, c_zn, c_zo))
    S_r = _mag(res) + _mag(x0)
    S_y = _mag(y) + step * S_r
    S_z = c_z * _mag(y) + _mag(x) + c_y * S_y
    S_x = c_x * _mag(x) + c_zn * S_z + c_zo * _mag(z)
    return {"res": gam(1) * S_r,             # one subtraction
            "y": gam(3 + kp) * S_y,          # res (1), step res (1), y - . (1), the prox
            "z": gam(6 + kp) * S_z,          # y (3 + k_prox), the two products (1), two additions (2)
            "x": gam(9 + kp) * S_x}          # z (6 + k_prox), the three products (1), two additions (2)


def pogm_gates(res, x0, xbuf, ybuf, z, rho, c_y, c_x1, c_xo, c_z, reg_kind, thr, proj_kind, rg):
    """per element bounds of res, xbuf, z, ybuf, w (module docstring)"""
    kp = k_prox(reg_kind, np.iscomplexobj(xbuf))
    rho, c_y, c_x1, c_xo, c_z, rg = (abs(float(c)) for c in (rho, c_y, c_x1, c_xo, c_z, rg))
    S_r = _mag(res) + _mag(x0)
    S_1 = _mag(xbuf) + rho * S_r
    S_z = c_y * _mag(ybuf) + c_x1 * S_1 + c_xo * _mag(xbuf) + c_z * _mag(z)
    S_w = 2.0 * rg * S_z + S_1
    return {"res": gam(1) * S_r,             # one subtraction
            "xbuf": gam(3) * S_1,            # res (1), rho res (1), x - . (1)
            "z": gam(7) * S_z,               # x1 (3), the four products (1), three additions (2 + 1)
            "ybuf": gam(7 + kp) * S_z,       # z, the prox; the projections round nothing
            "w": gam(10 + kp) * S_w}         # x (7 + k_prox; z and x1 bring less), the products (1), two subtractions (2)


def sum_gate(want, n, sum_abs):
    return U * abs(float(want)) + (n + 4) * 2.0 ** -53 * float(sum_abs)


def norm_gate(res_got):
    """(want, bound) of ||res|| from the res vector that came back: the double sum of squares is within (n + 4) 2^-53 of itself,
    its root within half of that, relatively; then the one rounding to Float32"""
    want = np.sqrt(redot(res_got, res_got))
    return float(want), sum_gate(want, res_got.size, want)


def dot_gates(w_in, out, rg):
    """{name: (want, bound)} of the three dot products from the vectors that came back (`out`: res, xbuf, ybuf, z)"""
    hi = np.complex128 if np.iscomplexobj(out["z"]) else np.float64
    w, x1, xn, zn, r = (np.asarray(v).astype(hi) for v in (w_in, out["xbuf"], out["ybuf"], out["z"], out["res"]))
    rg = float(rg)
    wi = w + x1 + rg * xn - rg * zn
    S_w = _mag(w) + _mag(x1) + abs(rg) * (_mag(xn) + _mag(zn))
    gates = {}
    for name, v in (("dwx", xn), ("dwz", zn), ("dwr", r)):
        want = redot(wi, v)
        gates[name] = (float(want), sum_gate(want, v.size, np.sum(_mag(wi) * _mag(v))) + float(np.sum(gam(4) * S_w * _mag(v))))
    return gates


# ---- the inputs of the kernel-level cases ------------------------------------------------------------------------------------------------
LENGTHS = [1, 63, 64, 1023, 1024, 1025, 5000]     # for (i = threadIdx.x; i < n; i += 1024): below a wave, a wave, below / at / past one pass, five passes
FULL_CROSS_N = 1025
_iter3 = {}


def iteration3(solver, dt):
    """the state scalars of the Float32 oracle after three iterations of a 24 x 16 solve (theta, sigma, gamma, theta_n, rho, lambda):
    the coefficients of the cases are those of its fourth iteration -- mixed signs, O(1)"""
    import rls_oracle as O

    key = (solver, np.dtype(dt))
    if key not in _iter3:
        A, _, b = O.make_problem(24, 16, dt, 7)
        hi = np.complex128 if np.dtype(dt).kind == "c" else np.float64
        rho = np.float32(0.9 / np.linalg.norm(A.astype(hi), 2) ** 2)
        lam = np.float32(0.05)
        kw = {"restart": "gradient", "sigma_fac": 0.96} if solver == "POGM-restart" else {}
        S = getattr(O, solver.split("-")[0])(A, reg=O.L1Regularization(lam), rho=rho, iterations=8, relTol=0.0, **kw)
        S.init(b)
        for _ in range(3):
            S.iterate()
        _iter3[key] = {"theta": np.float32(S.theta), "sigma": np.float32(getattr(S, "sigma", 1)), "gamma": np.float32(S.gamma),
                       "theta_n": np.float32(getattr(S, "theta_n", 0)), "rho": rho, "lam": lam}
    return _iter3[key]


def vector(dt, n, seed):
    rng = np.random.default_rng(seed)
    v = rng.standard_normal(n)
    if np.dtype(dt).kind == "c":
        v = (v + 1j * rng.standard_normal(n)) / math.sqrt(2.0)
    return v.astype(dt)


def _unit(dt, k):
    """a direction of modulus one with a negative real part (complex: off both axes)"""
    return np.dtype(dt).type(np.exp(1j * (2.2 + 0.3 * k))) if np.dtype(dt).kind == "c" else np.dtype(dt).type(-1)


def optista_case(dt, n, reg_kind=REG_L1, seed=0):
    """(vectors on entry, the ABI's coefficients).  Planted where n allows, by the prox input v = y - step (res - x0):
       0  negative real part, modulus 5 thr with every operand of that size (the eps of the L1 prox is an absolute 2^-23: it shows
          against small magnitudes only)
       1  exactly zero (y = 0, res = x0)
       2  modulus thr / 2
       3  thr (1 + 3 ulp) (res = x0: v = y exactly)"""
    s = iteration3("OptISTA", dt)
    c = optista_coefs(s["theta"], s["theta_n"], False, s["rho"], s["lam"])
    c = {k: np.float32(c[k]) for k in ("step", "thr", "c_z", "c_y", "c_x", "c_zn", "c_zo")}
    c["reg_kind"] = reg_kind
    v = {name: vector(dt, n, 1000 * n + 10 * seed + i) for i, name in enumerate(("res", "x0", "x", "y", "z"))}
    thr, T = c["thr"], np.float32
    small = {name: (thr * vector(dt, 4, 77 + i)).astype(dt) for i, name in enumerate(("res", "x0", "x", "y", "z"))}
    for i in range(min(n, 4)):
        for name in v:
            v[name][i] = small[name][i]
    v["y"][0] = T(5) * thr * _unit(dt, 0)
    if n > 1:
        v["y"][1], v["res"][1] = 0, v["x0"][1]
    if n > 2:
        v["y"][2], v["res"][2] = T(0.5) * thr * _unit(dt, 2), v["x0"][2]
    if n > 3:
        v["y"][3], v["res"][3] = np.nextafter(np.nextafter(np.nextafter(thr, T(1)), T(1)), T(1)), v["x0"][3]
    return v, c


def pogm_case(dt, n, reg_kind=REG_L1, proj_kind=PROJ_POSITIVE, restart=True, seed=0, solver="POGM-restart"):
    """as optista_case, by the prox input v = c_y ybuf + c_x1 (xbuf - rho (res - x0)) + c_xo xbuf + c_z z:
       0  negative real part, modulus about 5 thr, every operand of that size
       1  exactly zero (every operand zero, res = x0)
       2  modulus thr / 2        (xbuf = z = 0, res = x0: v = c_y ybuf)
       3  within 2 ulp of thr    (the same, ybuf = thr (1 + 3 ulp) / c_y)"""
    s = iteration3(solver, dt)
    c = pogm_coefs(s["theta"], s["sigma"], s["gamma"], False, s["rho"], s["lam"], restart)
    c = {k: np.float32(c[k]) for k in ("rho", "c_y", "c_x1", "c_xo", "c_z", "thr", "rg")}
    c.update(reg_kind=reg_kind, proj_kind=proj_kind, restart=int(restart))
    names = ("res", "x0", "xbuf", "ybuf", "z", "w")
    v = {name: vector(dt, n, 2000 * n + 10 * seed + i) for i, name in enumerate(names)}
    thr, T = c["thr"], np.float32
    small = {name: (thr * vector(dt, 4, 177 + i)).astype(dt) for i, name in enumerate(names)}
    for i in range(min(n, 4)):
        for name in v:
            v[name][i] = small[name][i]
    for i in range(1, min(n, 4)):
        v["xbuf"][i] = v["z"][i] = 0
        v["res"][i] = v["x0"][i]
    v["ybuf"][0] = T(5) * thr / c["c_y"] * _unit(dt, 0) * T(-1 if c["c_y"] < 0 else 1)
    if n > 1:
        v["ybuf"][1] = 0
    if n > 2:
        v["ybuf"][2] = T(0.5) * thr / c["c_y"] * _unit(dt, 2)
    if n > 3:
        v["ybuf"][3] = np.nextafter(np.nextafter(np.nextafter(thr, T(1)), T(1)), T(1)) / abs(c["c_y"])
    return v, c


def optista_args(c):
    return (c["step"], c["reg_kind"], c["thr"], c["c_z"], c["c_y"], c["c_x"], c["c_zn"], c["c_zo"])


def pogm_args(c):
    return (c["rho"], c["c_y"], c["c_x1"], c["c_xo"], c["c_z"], c["reg_kind"], c["thr"], c["proj_kind"], c["restart"], c["rg"])


def check_vectors(held, group, case, got, want, gates, exact=()):
    """every gated output of `got` against `want` within `gates`; the copies bit for bit"""
    for name, bound in gates.items():
        if want.get(name) is None or got.get(name) is None:
            continue
        err = np.abs(np.asarray(got[name]).astype(np.complex128) - np.asarray(want[name]).astype(np.complex128))
        held(f"{group} {name}", case, err, bound)
    for name in exact:
        assert np.asarray(got[name]).tobytes() == np.asarray(want[name]).astype(np.asarray(got[name]).dtype).tobytes(), (group, case, name)
