"""The fused backward pass robots / plan <- solve without a GPU: its numpy
statement tests/srbd_solve_vjp_host.py (descriptor from the vectors, the adjoint by projection)
against the chained one (adjoint_rows_host's outer products, then linearize_vjp), the argument
checks of srbd_qp_srbd_solve_backward_f64 in the header's order, and the ctypes mirror."""
import ctypes as C
import re

import numpy as np
import pytest

import adjoint_rows_host as arh
import helpers
import linearize_backward_cases as LC
import linearize_vjp_host as VH
import robots_host as BH
import srbd_solve_vjp_host as SH

EINVAL, EDIM, ECAPACITY, ESETTINGS = -1, -2, -5, -6
SYMBOL = "srbd_qp_srbd_solve_backward_f64"
B, N = 3, 3
BOUND = 1e-9  # |fused - chain| <= BOUND max|chain|: two statements of one quantity
# the forward solve's settings and the active-set tolerances of tests/test_gpu_linearize_backward.py
ST = dict(mode="Speed", iter_max=100, alpha_min=1e-8, mu0=1e2, tol_stat=1e-8, tol_eq=1e-8, tol_ineq=1e-8,
          tol_comp=1e-8, reg_prim=0.0, warm_start=0, pred_corr=1, ric_alg=0, split_step=1)
ACT_TOL, RANK_TOL = 1e-4, 1e-8


def host_qp(sm, OcpQpBatch, params, plan, xs, us, constraints):
    """The linearisation's QP as an OcpQpBatch (math orientation)."""
    pk = BH.build_qp(sm, params, xs, us, constraints, plan)
    n, Nn = xs.shape[0], us.shape[1]
    mat = lambda k, rows: np.swapaxes(pk[k].reshape(n, -1, 12, rows), -1, -2)
    kw = dict(N=Nn, nx=12, nu=12, A=mat("A", 12), B=mat("B", 12), b=pk["b"], Q=mat("Q", 12), S=mat("S", 12),
              R=mat("R", 12), q=pk["q"], r=pk["r"])
    if constraints == "box_u":
        kw.update(lbu=pk["lbu"], ubu=pk["ubu"])
    elif constraints == "cone":
        kw.update(ng=24, D=mat("D", 24), lg=pk["lg"], ug=pk["ug"], lg_mask=pk["lg_mask"], ug_mask=pk["ug_mask"])
    return OcpQpBatch(**kw)


def chained(sm, qp, params, plan, xs, us, constraints, x, u, pi, gx, gu):
    """adjoint_rows_host -> linearize_vjp: (the ten gradients and x0, active inputs + rows)."""
    cot = {k: [] for k in VH.COTANGENTS[constraints]}
    gx0, active = [], 0
    for i in range(xs.shape[0]):
        g, counts = arh.adjoint_rows_host(qp, x[i], u[i], pi[i], gx[i], gu[i], i, ACT_TOL, RANK_TOL)
        active += counts[0] + counts[1]
        gx0.append(g["x0"])
        for k in cot:  # math orientation -> the packed column-major blocks
            cot[k].append(np.swapaxes(g[k], -1, -2) if g[k].ndim == 3 else g[k])
    out = VH.linearize_vjp(sm, params, xs, us, constraints, {k: np.ascontiguousarray(np.array(v)) for k, v in cot.items()},
                           plan)
    out["x0"] = np.array(gx0)
    return out, active


def fused(sm, qp, params, plan, xs, us, constraints, x, u, pi, gx, gu):
    per = [SH.adjoint_vectors(qp, x[i], u[i], pi[i], gx[i], gu[i], i, ACT_TOL, RANK_TOL) for i in range(xs.shape[0])]
    vecs = {k: np.array([v[k] for v in per]) for k in ("dx", "du", "dpi", "nu", "dnu", "gubu")}
    vecs.update(x=x, u=u, pi=pi)
    return SH.solve_vjp(sm, params, xs, us, constraints, vecs, plan), sum(v["counts"][0] + v["counts"][1] for v in per)


@pytest.mark.parametrize("given", ["robots and plan", "neither"])
@pytest.mark.parametrize("constraints", ["none", "box_u", "cone"])
def test_fused_statement_matches_the_chained_one(pkg, oracle, OcpQpBatch, constraints, given):
    """Seen (largest |fused - chain| / max|chain| over the six cases and eleven outputs): 3.7e-14
    (foot_r, box_u with robots and plan); without an active set the two agree to 4e-16."""
    sm = pkg.srbd_model
    both = given == "robots and plan"
    p, params, plan, xs, us = LC.make_case(sm, B, N, robots=BH.MODEL_FIELDS if both else (),
                                           plan=LC.PLAN_FIELDS if both else ())
    _, _, x0 = sm.sample_trajectories(B, N, 4321, p)
    qp = host_qp(sm, OcpQpBatch, params, plan, xs, us, constraints)
    fwd = oracle.solve(qp, ST, x0=x0, riccati=False)
    assert np.all(fwd["status"] == 0), fwd["status"]
    x, u, pi = fwd["x"], fwd["u"], fwd["pi"]
    gx, gu = 2.0 * x, 2.0 * u  # loss = sum x^2 + sum u^2
    want, active = chained(sm, qp, params, plan, xs, us, constraints, x, u, pi, gx, gu)
    got, active_f = fused(sm, qp, params, plan, xs, us, constraints, x, u, pi, gx, gu)
    assert active == active_f
    if constraints != "none" and both:  # the plan's swing feet (fz_max = 1) put bounds and rows on the active set
        assert active > 0, "no bound or row is active: the constrained path is not exercised"
    for name in SH.OUTPUTS + ("x0",):
        scale = np.abs(want[name]).max()
        err = np.abs(got[name] - want[name]).max()
        print(f"[srbd solve backward] {constraints} {given} {name}: max|chain| {scale:.3g}, error / max "
              f"{err / scale if scale > 0 else 0.0:.2e}")
        assert err <= BOUND * scale, (name, err, scale)


def test_symbol_is_exported_and_bound(pkg):
    capi = pkg.capi
    assert SYMBOL in capi.exported_symbols() and SYMBOL in capi.PROTOTYPES
    assert hasattr(capi.lib(), SYMBOL)
    assert capi.lib().srbd_qp_abi_version() == 12  # additive to ABI 12
    assert hasattr(capi, "srbd_solve_backward") and hasattr(capi.Handle, "srbd_solve_backward_device")
    assert hasattr(pkg.diff, "srbd_solve")


def test_ctypes_mirror_is_the_headers_prototype(pkg):
    """The argument list of the header's declaration, type by type, against capi.PROTOTYPES."""
    capi = pkg.capi
    hdr = (helpers.REPO / "include" / "srbd_qp.h").read_text()
    decl = re.search(r"int " + SYMBOL + r"\((.*?)\);", hdr, re.S).group(1)
    decl = re.sub(r"/\*.*?\*/", "", decl, flags=re.S)
    P, vp = C.POINTER, C.c_void_p
    kinds = {"srbd_qp_handle": vp, "int": C.c_int, "double": C.c_double, "const srbd_qp_settings*": P(capi.Settings),
             "const srbd_model_params*": P(capi.ModelParams), "const srbd_plan_f64*": P(capi.PlanStruct),
             "const double*": vp, "double*": vp, "void*": vp, "const srbd_qp_data_f64*": P(capi.Data),
             "const srbd_qp_solution_f64*": P(capi.Solution), "const srbd_lin_grad_f64*": P(capi.LinGrad)}
    types, names = [], []
    for arg in decl.split(","):
        m = re.fullmatch(r"\s*(.*?)\s*(\w+)\s*", arg, re.S)
        types.append(kinds[" ".join(m.group(1).split())])
        names.append(m.group(2))
    assert names == ["h", "batch", "settings", "params", "plan", "constraints", "xs", "us", "data", "sol", "gx", "gu",
                     "act_tol", "rank_tol", "grad", "grad_x0", "stream"]
    restype, argtypes, _ = capi.PROTOTYPES[SYMBOL]
    assert restype is C.c_int and argtypes == types


def _fake_handle(dims, capacity):
    """Memory that begins like the library's handle (dims, then capacity): the checks below are
    all made before any device work and read nothing else of it."""
    buf = C.create_string_buffer(1 << 16)
    C.memmove(buf, C.byref(dims), C.sizeof(dims))
    C.memmove(C.byref(buf, C.sizeof(dims)), C.byref(C.c_int(capacity)), C.sizeof(C.c_int))
    return buf


def test_argument_checks_in_the_headers_order(pkg):
    capi = pkg.capi
    L = capi.lib()
    p, plan, st = capi.default_model_params(), capi.PlanStruct(), capi.settings_struct(ST)
    none, one = capi.LinGrad(), capi.LinGrad(mass=8)
    a = C.c_void_p(16)
    full = capi.Data(**{k: 16 for k in ("A", "B", "b", "Q", "S", "R", "q", "r", "x0")})
    sol = capi.Solution(x=16, u=16, pi=16)
    h0 = _fake_handle(capi.Dims(N, 12, 12, 0, 0, 0, 0), 4)
    last = lambda: L.srbd_qp_last_error().decode()

    def call(h=h0, batch=1, st=C.byref(st), params=C.byref(p), constraints=0, xs=a, us=a, data=C.byref(full),
             sol=C.byref(sol), gx=a, gu=a, act_tol=1e-4, rank_tol=1e-8, grad=C.byref(one), gx0=None):
        h = C.cast(h, C.c_void_p) if h is not None else None
        return getattr(L, SYMBOL)(h, batch, st, params, C.byref(plan), constraints, xs, us, data, sol, gx, gu,
                                  C.c_double(act_tol), C.c_double(rank_tol), grad, gx0, None)

    # 1. the linearisation's checks come first, whatever else is wrong
    bad = dict(st=None, data=None, act_tol=-1.0)
    for kw in (dict(h=None), dict(params=None), dict(xs=None), dict(us=None), dict(grad=None)):
        assert call(batch=99, constraints=7, **bad, **kw) == EINVAL, kw
        assert "NULL argument" in last()
    assert call(h=_fake_handle(capi.Dims(N, 13, 12, 0, 0, 0, 0), 4), batch=99, constraints=7, **bad) == EDIM
    assert call(batch=5, constraints=7, **bad) == ECAPACITY
    assert call(batch=-1, constraints=7, **bad) == ECAPACITY
    for mode in (-1, 3):
        assert call(constraints=mode, **bad) == EINVAL and "constraints" in last()
    assert call(constraints=2, **bad) == EINVAL and "ng = 24" in last()
    # 2. then those of srbd_qp_solve_backward_rows_f64, in its order -- before the outputs
    nothing = dict(grad=C.byref(none))
    assert call(data=None, st=None, **nothing) == EINVAL and "data/solution/grad" in last()
    assert call(sol=None, st=None, **nothing) == EINVAL and "data/solution/grad" in last()
    assert call(st=None, gx=None, gu=None, **nothing) == EINVAL and "settings is NULL" in last()
    assert call(gx=None, gu=None, act_tol=-1.0, **nothing) == EINVAL and "no cotangent" in last()
    assert call(act_tol=-1.0, rank_tol=1.0, **nothing) == EINVAL and "act_tol" in last()
    assert call(act_tol=float("inf"), **nothing) == EINVAL and "act_tol" in last()
    assert call(rank_tol=1.0, **nothing) == EINVAL and "rank_tol" in last()
    neg = capi.settings_struct(dict(ST, reg_prim=-1.0))
    assert call(st=C.byref(neg), **nothing) == ESETTINGS
    h24 = _fake_handle(capi.Dims(N, 12, 12, 24, 0, 0, 0), 4)
    rows = capi.Data.from_buffer_copy(full)
    rows.D = rows.lg = rows.ug = 16
    with_c = capi.Data.from_buffer_copy(rows)
    with_c.C = 16
    assert call(h=h24, constraints=2, data=C.byref(with_c), **nothing) == EDIM and "C != NULL" in last()
    assert call(h=_fake_handle(capi.Dims(N, 12, 12, 0, 0, 1, 0), 4), **nothing) == EDIM and "has_box_x" in last()
    assert call(h=_fake_handle(capi.Dims(N, 12, 12, 0, 0, 0, 1), 4), **nothing) == EDIM and "stage-major" in last()
    no_q = capi.Data.from_buffer_copy(full)
    no_q.Q = None
    assert call(data=C.byref(no_q), **nothing) == EINVAL and "are required" in last()
    assert call(sol=C.byref(capi.Solution(x=16, u=16)), **nothing) == EINVAL and "forward x, u and pi" in last()
    hbox = _fake_handle(capi.Dims(N, 12, 12, 0, 1, 0, 0), 4)
    assert call(h=hbox, constraints=1, **nothing) == EINVAL and "lbu and ubu" in last()
    assert call(h=h24, constraints=2, **nothing) == EINVAL and "D, lg and ug" in last()
    # 3. every output NULL and no grad_x0 -- before batch == 0
    assert call(batch=0, **nothing) == EINVAL and "grad" in last()
    # 4. batch == 0 is a success that does nothing (with grad_x0 alone too, and the cone)
    assert call(batch=0) == 0
    assert call(batch=0, gx0=a, **nothing) == 0
    assert call(h=h24, batch=0, constraints=2, data=C.byref(rows)) == 0


def test_binding_checks_its_tensors(pkg):
    import types

    import torch
    capi = pkg.capi
    handle = types.SimpleNamespace(dims=capi.Dims(N, 12, 12, 0, 0, 0, 0), device=0)
    xs, us = torch.zeros(B, N + 1, 12, dtype=torch.float64), torch.zeros(B, N, 12, dtype=torch.float64)
    data, sol = capi.Data(), capi.Solution()
    with pytest.raises(ValueError, match="xs is on cpu"):
        capi.srbd_solve_backward(handle, xs, us, data, sol, None, None)
    with pytest.raises(ValueError, match="xs must be"):
        capi.srbd_solve_backward(handle, xs.float(), us, data, sol, None, None)
    with pytest.raises(ValueError, match="unknown constraints"):
        capi.srbd_solve_backward(handle, xs, us, data, sol, None, None, constraints="soft")
