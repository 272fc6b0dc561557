"""The batched QP solve as a differentiable torch function (srbd_qp_solve_f64 forward,
srbd_qp_solve_backward_f64 backward).

    x, u, pi = solve_qp(handle, A, B, b, Q, S, R, q, r, x0)
    loss(x, u).backward()        # A.grad, ..., x0.grad for the inputs that require grad

Both passes run the HIP kernels on the handle's device; nothing is computed by torch.
"""
from __future__ import annotations

import math

from . import capi

__all__ = ["solve_qp"]

_INPUTS = capi.GRAD_FIELDS  # A, B, b, Q, S, R, q, r, x0: the differentiable inputs, in this order
_BOUNDS = ("lbu", "ubu", "lbu_mask", "ubu_mask")


def _shapes(dims):
    N, nx, nu = dims.N, dims.nx, dims.nu
    return {"A": (N, nx, nx), "B": (N, nu, nx), "b": (N, nx), "Q": (N + 1, nx, nx), "S": (N, nx, nu),
            "R": (N, nu, nu), "q": (N + 1, nx), "r": (N, nu), "x0": (nx,),
            "lbu": (N, nu), "ubu": (N, nu), "lbu_mask": (N, nu), "ubu_mask": (N, nu)}


def _make_function():
    import torch

    class _SolveQp(torch.autograd.Function):
        @staticmethod
        def forward(ctx, handle, settings, act_tol, *tensors):
            named = dict(zip(_INPUTS + _BOUNDS, tensors))
            A = named["A"]
            batch, dims = A.shape[0], handle.dims
            new = lambda *shape: torch.zeros(batch, *shape, dtype=torch.float64, device=A.device)
            x, u, pi = new(dims.N + 1, dims.nx), new(dims.N, dims.nu), new(dims.N + 1, dims.nx)
            data = capi.Data(**{k: capi._tensor_ptr(named.get(k)) or None for k in capi.DATA_FIELDS})
            sol = capi.Solution(x=x.data_ptr(), u=u.data_ptr(), pi=pi.data_ptr())
            handle.solve_device(batch, settings, data, sol)
            ctx.handle, ctx.settings, ctx.act_tol = handle, settings, act_tol
            ctx.save_for_backward(*[t for t in tensors if t is not None], x, u, pi)
            ctx.present = [t is not None for t in tensors]
            ctx.mark_non_differentiable(pi)
            return x, u, pi

        @staticmethod
        def backward(ctx, gx, gu, _gpi):
            saved = list(ctx.saved_tensors)
            x, u, pi = saved[-3:]
            it = iter(saved[:-3])
            named = dict(zip(_INPUTS + _BOUNDS, [next(it) if p else None for p in ctx.present]))
            none = (None,) * (3 + len(_INPUTS) + len(_BOUNDS))
            if gx is None and gu is None:
                return none
            # (handle, settings, act_tol) come first in forward's arguments
            wanted = [n for n, need in zip(_INPUTS, ctx.needs_input_grad[3:3 + len(_INPUTS)]) if need]
            if not wanted:
                return none
            gx = None if gx is None else gx.contiguous()
            gu = None if gu is None else gu.contiguous()
            out = {n: torch.empty_like(named[n]) for n in wanted}
            batch = x.shape[0]
            data = capi.Data(**{k: capi._tensor_ptr(named.get(k)) or None for k in capi.DATA_FIELDS})
            sol = capi.Solution(x=x.data_ptr(), u=u.data_ptr(), pi=pi.data_ptr())
            grad = capi.Grad(**{n: t.data_ptr() for n, t in out.items()})
            ctx.handle.solve_backward_device(batch, ctx.settings, data, sol, gx, gu, grad, act_tol=ctx.act_tol)
            return (None, None, None) + tuple(out.get(n) for n in _INPUTS) + (None,) * len(_BOUNDS)

    return _SolveQp


_function = None


def solve_qp(handle, A, B, b, Q, S, R, q, r, x0, lbu=None, ubu=None, lbu_mask=None, ubu_mask=None,
             settings=None, act_tol=None):
    """Solve a batch of OCP-QPs on `handle` (a capi.Handle without general rows and state boxes)
    and return (x, u, pi), differentiable with respect to A, B, b, Q, S, R, q, r and x0.

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
    has_box_u; they get no gradient.  The backward pass then holds the active set fixed: an input
    within act_tol of an unmasked bound is pinned (default sqrt(tol_comp), the slack at which a
    bound's slack and multiplier are equal when the IPM stops).
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
                 ubu_mask=ubu_mask)
    shapes = _shapes(handle.dims)
    batch = None
    for name, t in given.items():
        if t is None:
            if name not in _BOUNDS:
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
    if act_tol is None:
        act_tol = math.sqrt(st.tol_comp)
    return _function.apply(handle, st, float(act_tol), *[given[n] for n in _INPUTS + _BOUNDS])
