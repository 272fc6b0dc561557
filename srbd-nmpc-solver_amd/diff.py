"""The batched QP solve as a differentiable torch function (srbd_qp_solve_f64 forward,
srbd_qp_solve_backward_f64 or srbd_qp_solve_backward_rows_f64 backward).

    x, u, pi = solve_qp(handle, A, B, b, Q, S, R, q, r, x0)
    loss(x, u).backward()        # A.grad, ..., x0.grad for the inputs that require grad

With general rows on the inputs (a handle with ng > 0) D, lg, ug are inputs too, and they and
lbu, ubu receive gradients.

srbd_linearize is the link before it: the SRBD linearisation as a differentiable function of the
handle's robots and of the plan (srbd_qp_srbd_linearize_plan_f64 forward,
srbd_qp_srbd_linearize_backward_f64 backward), so that

    qp = srbd_linearize(handle, xs, us, plan=plan)
    x, u, pi = solve_qp(handle, x0=x0, **{k: qp[k] for k in ("A", "B", "b", "Q", "S", "R", "q", "r")})
    loss(x, u).backward()        # robots.mass.grad, robots.Q.grad, plan.fz_max.grad, ...

srbd_solve is the two in one function with one backward call (srbd_qp_srbd_solve_backward_f64;
DESIGN.md 4.13d): the gradients of the QP arrays are never formed or held.

    x, u, pi = srbd_solve(handle, xs, us, x0, plan=plan)
    loss(x, u).backward()        # robots.mass.grad, ..., plan.fz_max.grad, x0.grad

plant_rollout is the true robot's side: the open-loop plant rollout as a differentiable function of
its start, inputs, feet and wrench and of the plant's mass and inertia (srbd_qp_srbd_plant_rollout_f64
forward, srbd_qp_srbd_plant_rollout_backward_f64 backward).

    x_traj = plant_rollout(handle, x0, u_log, foot_r, foot_l, wrench)
    ((x_traj - x_log) ** 2).sum().backward()   # plant.mass.grad, plant.Lbody.grad, u_log.grad, ...

All passes run the HIP kernels on the handle's device; nothing is computed by torch.
"""
from __future__ import annotations

import math

from . import capi

__all__ = ["solve_qp", "srbd_linearize", "srbd_solve", "plant_rollout"]

_INPUTS = capi.GRAD_FIELDS  # A, B, b, Q, S, R, q, r, x0: the differentiable inputs, in this order
_BOUNDS = ("lbu", "ubu", "lbu_mask", "ubu_mask")
_ROWS = ("D", "lg", "ug", "lg_mask", "ug_mask")
_TENSORS = _INPUTS + _BOUNDS + _ROWS
_ROW_GRADS = capi.GRAD_ROWS_FIELDS  # D, lg, ug, lbu, ubu: differentiable through the rows entry point
_LEAD = 4  # forward's arguments before the tensors: handle, settings, act_tol, rank_tol


def _shapes(dims):
    N, nx, nu, ng = dims.N, dims.nx, dims.nu, dims.ng
    rows = {"D": (N, nu, ng), "lg": (N + 1, ng), "ug": (N + 1, ng), "lg_mask": (N + 1, ng), "ug_mask": (N + 1, ng)}
    return {**rows, "A": (N, nx, nx), "B": (N, nu, nx), "b": (N, nx), "Q": (N + 1, nx, nx), "S": (N, nx, nu),
            "R": (N, nu, nu), "q": (N + 1, nx), "r": (N, nu), "x0": (nx,),
            "lbu": (N, nu), "ubu": (N, nu), "lbu_mask": (N, nu), "ubu_mask": (N, nu)}


def _make_function():
    import torch

    class _SolveQp(torch.autograd.Function):
        @staticmethod
        def forward(ctx, handle, settings, act_tol, rank_tol, *tensors):
            named = dict(zip(_TENSORS, tensors))
            A = named["A"]
            batch, dims = A.shape[0], handle.dims
            new = lambda *shape: torch.zeros(batch, *shape, dtype=torch.float64, device=A.device)
            x, u, pi = new(dims.N + 1, dims.nx), new(dims.N, dims.nu), new(dims.N + 1, dims.nx)
            data = capi.Data(**{k: capi._tensor_ptr(named.get(k)) or None for k in capi.DATA_FIELDS})
            sol = capi.Solution(x=x.data_ptr(), u=u.data_ptr(), pi=pi.data_ptr())
            handle.solve_device(batch, settings, data, sol)
            ctx.handle, ctx.settings, ctx.act_tol, ctx.rank_tol = handle, settings, act_tol, rank_tol
            ctx.save_for_backward(*[t for t in tensors if t is not None], x, u, pi)
            ctx.present = [t is not None for t in tensors]
            ctx.mark_non_differentiable(pi)
            return x, u, pi

        @staticmethod
        def backward(ctx, gx, gu, _gpi):
            saved = list(ctx.saved_tensors)
            x, u, pi = saved[-3:]
            it = iter(saved[:-3])
            named = dict(zip(_TENSORS, [next(it) if p else None for p in ctx.present]))
            none = (None,) * (_LEAD + len(_TENSORS))
            if gx is None and gu is None:
                return none
            needs = dict(zip(_TENSORS, ctx.needs_input_grad[_LEAD:]))
            wanted = [n for n in _INPUTS if needs[n]]
            wanted_rows = [n for n in _ROW_GRADS if needs[n]]
            if not wanted and not wanted_rows:
                return none
            gx = None if gx is None else gx.contiguous()
            gu = None if gu is None else gu.contiguous()
            out = {n: torch.empty_like(named[n]) for n in wanted + wanted_rows}
            batch = x.shape[0]
            data = capi.Data(**{k: capi._tensor_ptr(named.get(k)) or None for k in capi.DATA_FIELDS})
            sol = capi.Solution(x=x.data_ptr(), u=u.data_ptr(), pi=pi.data_ptr())
            grad = capi.Grad(**{n: out[n].data_ptr() for n in wanted})
            if ctx.handle.dims.ng > 0 or wanted_rows:
                rows = capi.GradRows(**{n: out[n].data_ptr() for n in wanted_rows})
                ctx.handle.solve_backward_rows_device(batch, ctx.settings, data, sol, gx, gu, grad if wanted else None,
                                                      rows if wanted_rows else None, act_tol=ctx.act_tol,
                                                      rank_tol=ctx.rank_tol)
            else:  # nothing of the rows: the entry point without them
                ctx.handle.solve_backward_device(batch, ctx.settings, data, sol, gx, gu, grad, act_tol=ctx.act_tol)
            return (None,) * _LEAD + tuple(out.get(n) for n in _TENSORS)

    return _SolveQp


_function = None


def solve_qp(handle, A, B, b, Q, S, R, q, r, x0, lbu=None, ubu=None, lbu_mask=None, ubu_mask=None,
             settings=None, act_tol=None, D=None, lg=None, ug=None, lg_mask=None, ug_mask=None, rank_tol=1e-8):
    """Solve a batch of OCP-QPs on `handle` (a capi.Handle without state boxes and without rows
    on the states) and return (x, u, pi), differentiable with respect to A, B, b, Q, S, R, q, r and
    x0, and with respect to D, lg, ug, lbu and ubu.

    Every input is a contiguous torch.float64 tensor on the handle's device, in the C-ABI layout
    of include/srbd_qp.h, with a leading batch dimension:
        A [B][N][nx][nx]    B [B][N][nu][nx]    b [B][N][nx]
        Q [B][N+1][nx][nx]  S [B][N][nx][nu]    R [B][N][nu][nu]
        q [B][N+1][nx]      r [B][N][nu]        x0 [B][nx]
    Matrix blocks are column-major (qp.colmajor): as a row-major tensor each block is the
    transpose of the math matrix, so B's blocks have shape (nu, nx) and S's (nx, nu).  The
    gradients come back in the same layout.  Q.grad and R.grad are gradients with respect to a
    symmetric matrix: moving Q_ij and Q_ji together changes the loss by Q.grad_ij + Q.grad_ji.
    lbu, ubu (and the optional 0/1 masks) [B][N][nu] are the input box of a handle with
    has_box_u.  The backward pass then holds the active set fixed: an input within act_tol of an
    unmasked bound is pinned (default sqrt(tol_comp), the slack at which a bound's slack and
    multiplier are equal when the IPM stops).
    D [B][N][nu][ng] (column-major ng x nu blocks), lg, ug (and the optional 0/1 masks)
    [B][N+1][ng] are the general rows lg <= D u <= ug of a handle with ng > 0 (C = 0: rows on the
    inputs only).  A row within act_tol of an unmasked bound is active; active rows that depend on
    the pins and on the active rows before them (rank_tol) are dropped.  lbu, ubu, D, lg, ug get
    gradients; an inactive bound's is exactly zero.  The masks get none.
    settings: a dict for capi.settings_struct, a capi.Settings, or None for the defaults.
    x [B][N+1][nx], u [B][N][nu] carry gradients; pi [B][N+1][nx] is not differentiable.
    Tensors are checked here, with ValueError, before the library sees a pointer."""
    import torch
    global _function
    if _function is None:
        _function = _make_function()
    st = settings if isinstance(settings, capi.Settings) else capi.settings_struct(settings)
    device = torch.device("cuda", handle.device)
    given = dict(A=A, B=B, b=b, Q=Q, S=S, R=R, q=q, r=r, x0=x0, lbu=lbu, ubu=ubu, lbu_mask=lbu_mask,
                 ubu_mask=ubu_mask, D=D, lg=lg, ug=ug, lg_mask=lg_mask, ug_mask=ug_mask)
    shapes = _shapes(handle.dims)
    batch = None
    for name, t in given.items():
        if t is None:
            if name in _INPUTS:
                raise ValueError(f"{name} is required")
            continue
        capi._check_tensor(name, t, (torch.float64,), ("B",) + shapes[name], device, "the handle", any_gpu=True)
        if batch is not None and t.shape[0] != batch:
            raise ValueError(f"{name} has {t.shape[0]} QPs, A has {batch}")
        batch = t.shape[0]
    if (lbu is None) != (ubu is None) or (lbu is not None) != bool(handle.dims.has_box_u):
        raise ValueError("lbu and ubu go with a handle created with has_box_u, and only with one")
    if lbu is None and (lbu_mask is not None or ubu_mask is not None):
        raise ValueError("lbu_mask / ubu_mask need lbu and ubu")
    rows = [n for n in ("D", "lg", "ug") if given[n] is not None]
    if len(rows) not in (0, 3) or bool(rows) != (handle.dims.ng > 0):
        raise ValueError("D, lg and ug go with a handle created with ng > 0, and only with one")
    if not rows and (lg_mask is not None or ug_mask is not None):
        raise ValueError("lg_mask / ug_mask need D, lg and ug")
    if not (0.0 <= float(rank_tol) < 1.0):
        raise ValueError("rank_tol must be in [0, 1)")
    if act_tol is None:
        act_tol = math.sqrt(st.tol_comp)
    return _function.apply(handle, st, float(act_tol), float(rank_tol), *[given[n] for n in _TENSORS])


# ---- the linearisation ----
_LIN_SHAPES = {"A": (12, 12), "B": (12, 12), "b": (12,), "Q": (12, 12), "S": (12, 12), "R": (12, 12), "q": (12,),
               "r": (12,), "lbu": (12,), "ubu": (12,), "D": (12, 24), "lg": (24,), "ug": (24,), "lg_mask": (24,),
               "ug_mask": (24,)}
_LIN_OUT = {"none": ("A", "B", "b", "Q", "S", "R", "q", "r"),
            "box_u": ("A", "B", "b", "Q", "S", "R", "q", "r", "lbu", "ubu"),
            "cone": ("A", "B", "b", "Q", "S", "R", "q", "r", "D", "lg", "ug", "lg_mask", "ug_mask")}
_LIN_CONSTANT = ("S", "lbu", "ug", "lg_mask", "ug_mask")  # no parameter reaches them
_ROBOT_FIELDS = tuple(capi.Robots.FIELDS)  # mass, Lbody, mu, Q, Qf, R
_PLAN_FIELDS = tuple(capi.Plan.FIELDS)  # x_ref, foot_r, foot_l, fz_max
_LIN_LEAD = 7  # forward's arguments before the parameters: handle, constraints, params, plan, robots, xs, us


def _make_linearize():
    import torch

    class _SrbdLinearize(torch.autograd.Function):
        @staticmethod
        def forward(ctx, handle, constraints, params, plan, robots, xs, us, *leaves):
            t, _ = capi.srbd_linearize(handle, xs, us, constraints, params=params, plan=plan)
            ctx.handle, ctx.constraints, ctx.params, ctx.plan, ctx.robots = handle, constraints, params, plan, robots
            ctx.save_for_backward(xs, us)
            names = _LIN_OUT[constraints]
            outs = tuple(t[n].view(*t[n].shape[:2], *_LIN_SHAPES[n]) for n in names)
            ctx.mark_non_differentiable(*[o for n, o in zip(names, outs) if n in _LIN_CONSTANT])
            return outs

        @staticmethod
        def backward(ctx, *grads):
            none = (None,) * (_LIN_LEAD + len(_ROBOT_FIELDS) + len(_PLAN_FIELDS))
            names = _ROBOT_FIELDS + _PLAN_FIELDS
            want = [n for n, need in zip(names, ctx.needs_input_grad[_LIN_LEAD:]) if need]
            cot = {n: g.contiguous() for n, g in zip(_LIN_OUT[ctx.constraints], grads)
                   if g is not None and n not in _LIN_CONSTANT}
            if not want or not cot:
                return none
            if getattr(ctx.handle, "_robots", (None, None))[0] is not ctx.robots:
                raise RuntimeError("srbd_linearize: the handle's model robots were replaced (Handle.set_robots) "
                                   "between the forward and the backward pass")
            xs, us = ctx.saved_tensors
            out = capi.srbd_linearize_backward(ctx.handle, xs, us, cot, ctx.constraints, params=ctx.params,
                                               plan=ctx.plan, want=want)
            return none[:_LIN_LEAD] + tuple(out.get(n) for n in names)

    return _SrbdLinearize


_linearize = None


def srbd_linearize(handle, xs, us, constraints="none", params=None, plan=None):
    """capi.srbd_linearize as a differentiable function: the QP arrays of the SRBD linearisation at
    xs [B][N+1][12], us [B][N][12], as a dict of tensors in solve_qp's shapes (A, B, Q, S, R
    [B][N or N+1][12][12], b, q, r [..][12]; box_u: lbu, ubu [B][N][12]; cone: D [B][N][12][24], lg, ug
    and the masks [B][N+1][24]; column-major blocks, the C-ABI layout).
    Gradients go to those tensors of the handle's model robots (Handle.set_robots: mass, Lbody, mu,
    Q, Qf, R) and of `plan` (x_ref, foot_r, foot_l, fz_max) that require grad; xs and us get none
    (the linearisation point is held fixed), and S, lbu, ug and the masks are constants.  The
    backward pass raises RuntimeError if the handle's model robots are no longer the Robots object
    the forward call saw."""
    global _linearize
    if _linearize is None:
        _linearize = _make_linearize()
    if constraints not in _LIN_OUT:
        raise ValueError(f"unknown constraints {constraints!r}")
    robots = getattr(handle, "_robots", (None, None))[0]
    leaves = [None if robots is None else getattr(robots, n) for n in _ROBOT_FIELDS]
    leaves += [None if plan is None else getattr(plan, n) for n in _PLAN_FIELDS]
    outs = _linearize.apply(handle, constraints, params, plan, robots, xs, us, *leaves)
    return dict(zip(_LIN_OUT[constraints], outs))


# ---- linearise and solve in one function, the fused backward pass ----
# forward's arguments before the leaves: handle, constraints, params, plan, robots, settings, act_tol, rank_tol,
# xs, us, x0 (x0 is differentiable: the last of the lead)
_SOLVE_LEAD = 11


def _make_srbd_solve():
    import torch

    class _SrbdSolve(torch.autograd.Function):
        @staticmethod
        def forward(ctx, handle, constraints, params, plan, robots, settings, act_tol, rank_tol, xs, us, x0, *leaves):
            qp, data = capi.srbd_linearize(handle, xs, us, constraints, params=params, plan=plan)
            data.x0 = x0.data_ptr()
            batch, N = xs.shape[0], xs.shape[1] - 1
            new = lambda rows: torch.zeros(batch, rows, 12, dtype=torch.float64, device=xs.device)
            x, u, pi = new(N + 1), new(N), new(N + 1)
            handle.solve_device(batch, settings, data, capi.Solution(x=x.data_ptr(), u=u.data_ptr(), pi=pi.data_ptr()))
            ctx.handle, ctx.constraints, ctx.params, ctx.plan, ctx.robots = handle, constraints, params, plan, robots
            ctx.settings, ctx.act_tol, ctx.rank_tol = settings, act_tol, rank_tol
            ctx.qp = qp  # the QP arrays the backward pass reads: kept alive, not part of the graph
            ctx.save_for_backward(xs, us, x0, x, u, pi)
            ctx.mark_non_differentiable(pi)
            return x, u, pi

        @staticmethod
        def backward(ctx, gx, gu, _gpi):
            names = _ROBOT_FIELDS + _PLAN_FIELDS
            none = (None,) * (_SOLVE_LEAD + len(names))
            want = [n for n, need in zip(names, ctx.needs_input_grad[_SOLVE_LEAD:]) if need]
            want_x0 = ctx.needs_input_grad[_SOLVE_LEAD - 1]
            if (gx is None and gu is None) or not (want or want_x0):
                return none
            if getattr(ctx.handle, "_robots", (None, None))[0] is not ctx.robots:
                raise RuntimeError("srbd_solve: the handle's model robots were replaced (Handle.set_robots) "
                                   "between the forward and the backward pass")
            xs, us, x0, x, u, pi = ctx.saved_tensors
            data = capi.Data(**{k: capi._tensor_ptr(ctx.qp.get(k)) or None for k in capi.DATA_FIELDS})
            data.x0 = x0.data_ptr()
            sol = capi.Solution(x=x.data_ptr(), u=u.data_ptr(), pi=pi.data_ptr())
            out = capi.srbd_solve_backward(ctx.handle, xs, us, data, sol, None if gx is None else gx.contiguous(),
                                           None if gu is None else gu.contiguous(), ctx.constraints,
                                           params=ctx.params, plan=ctx.plan, act_tol=ctx.act_tol,
                                           rank_tol=ctx.rank_tol, want=want, settings=ctx.settings, want_x0=want_x0)
            return none[:_SOLVE_LEAD - 1] + (out.get("x0"),) + tuple(out.get(n) for n in names)

    return _SrbdSolve


_srbd_solve = None


def srbd_solve(handle, xs, us, x0, constraints="none", params=None, plan=None, settings=None, act_tol=None,
               rank_tol=1e-8):
    """srbd_linearize followed by solve_qp as one differentiable function with one backward call
    (srbd_qp_srbd_solve_backward_f64): the SRBD linearisation at xs [B][N+1][12], us [B][N][12] solved
    from x0 [B][12] on `handle` (created for the mode: has_box_u for "box_u", ng = 24 for "cone"),
    returning (x, u, pi).
    Gradients go to the leaves srbd_linearize finds -- the tensors of the handle's model robots
    (mass, Lbody, mu, Q, Qf, R) and of `plan` (x_ref, foot_r, foot_l, fz_max) that require grad --
    and to x0; xs and us get none.  The gradients of the QP arrays are never formed.  settings,
    act_tol, rank_tol: as in solve_qp.  The backward pass raises RuntimeError if the handle's model
    robots are no longer the Robots object the forward call saw."""
    import torch
    global _srbd_solve
    if _srbd_solve is None:
        _srbd_solve = _make_srbd_solve()
    if constraints not in _LIN_OUT:
        raise ValueError(f"unknown constraints {constraints!r}")
    st = settings if isinstance(settings, capi.Settings) else capi.settings_struct(settings)
    capi._check_tensor("xs", xs, (torch.float64,), ("B", None, 12), torch.device("cuda", handle.device), "the handle",
                       any_gpu=True)
    capi._check_tensor("x0", x0, (torch.float64,), (xs.shape[0], 12), xs.device)
    if not (0.0 <= float(rank_tol) < 1.0):
        raise ValueError("rank_tol must be in [0, 1)")
    if act_tol is None:
        act_tol = math.sqrt(st.tol_comp)
    robots = getattr(handle, "_robots", (None, None))[0]
    leaves = [None if robots is None else getattr(robots, n) for n in _ROBOT_FIELDS]
    leaves += [None if plan is None else getattr(plan, n) for n in _PLAN_FIELDS]
    return _srbd_solve.apply(handle, constraints, params, plan, robots, st, float(act_tol), float(rank_tol), xs, us,
                             x0, *leaves)


# ---- the plant: the open-loop rollout and its adjoint through time ----
# forward's arguments before the tensors: handle, params, substeps, roles
_PLANT_LEAD = 4
_PLANT_TENSORS = ("x0", "u", "foot_r", "foot_l", "wrench", "mass", "Lbody")  # capi.PLANT_GRAD_FIELDS' order


def _make_plant_rollout():
    import torch

    class _PlantRollout(torch.autograd.Function):
        @staticmethod
        def forward(ctx, handle, params, substeps, roles, x0, u, foot_r, foot_l, wrench, _mass, _Lbody):
            x_traj = capi.srbd_plant_rollout(handle, x0, u, foot_r, foot_l, wrench, substeps, params)
            ctx.handle, ctx.params, ctx.substeps, ctx.roles = handle, params, substeps, roles
            ctx.given = tuple(t is not None for t in (foot_r, foot_l, wrench))
            ctx.save_for_backward(x0, u, x_traj, *[t for t in (foot_r, foot_l, wrench) if t is not None])
            return x_traj

        @staticmethod
        def backward(ctx, gx):
            none = (None,) * (_PLANT_LEAD + len(_PLANT_TENSORS))
            want = [n for n, need in zip(_PLANT_TENSORS, ctx.needs_input_grad[_PLANT_LEAD:]) if need]
            if gx is None or not want:
                return none
            if getattr(ctx.handle, "_robots", (None, None)) != ctx.roles:
                raise RuntimeError("plant_rollout: the handle's robots were replaced (Handle.set_robots) between the "
                                   "forward and the backward pass")
            x0, u, x_traj, *rest = ctx.saved_tensors
            rest = iter(rest)
            foot_r, foot_l, wrench = (next(rest) if g else None for g in ctx.given)
            out = capi.srbd_plant_rollout_backward(ctx.handle, x0, u, foot_r, foot_l, wrench, ctx.substeps, ctx.params,
                                                   x_traj=x_traj, gx=gx.contiguous(), want=want)
            for name, foot in (("foot_r", foot_r), ("foot_l", foot_l)):  # a long plan's rows past T: zeros
                if name in out and foot.shape[1] > u.shape[1]:
                    full = torch.zeros_like(foot)
                    full[:, :u.shape[1]] = out[name]
                    out[name] = full
            return none[:_PLANT_LEAD] + tuple(out.get(n) for n in _PLANT_TENSORS)

    return _PlantRollout


_plant_rollout = None


def plant_rollout(handle, x0, u, foot_r=None, foot_l=None, wrench=None, substeps=1, params=None):
    """capi.srbd_plant_rollout as a differentiable function: x_traj [B][T+1][12], the true robot's
    states from x0 [B][12] under the inputs u [B][T][12], the feet foot_r / foot_l [B][P][3] (P >= T)
    and the wrench [B][T][6], each held over its tick.
    Gradients go to x0, u, foot_r, foot_l, wrench and to the mass / Lbody tensors the plant step
    resolves to -- per field the handle's plant robots' (Handle.set_robots), else its model robots'
    -- where they require grad; a foot tensor longer than T gets zeros in its rows past T.  The
    backward pass raises RuntimeError if either role is no longer the Robots object the forward
    call saw."""
    global _plant_rollout
    if _plant_rollout is None:
        _plant_rollout = _make_plant_rollout()
    roles = tuple(getattr(handle, "_robots", (None, None)))
    model, plant = roles
    leaf = lambda n: next((getattr(r, n) for r in (plant, model) if r is not None and getattr(r, n) is not None), None)
    return _plant_rollout.apply(handle, params, int(substeps), roles, x0, u, foot_r, foot_l, wrench, leaf("mass"),
                                leaf("Lbody"))
