"""ctypes binding of libsrbd_qp.so (the C-ABI declared in include/srbd_qp.h).

Device memory comes from torch (HIP tensors); every call goes through the
HIP kernels.  Importing this module on a host without the built library or
without a GPU works; calling a solve raises :class:`SrbdQpError`.
"""
from __future__ import annotations

import ctypes as C
import sys
import os
from pathlib import Path
from typing import Dict, Optional

import numpy as np

PKG_DIR = Path(__file__).resolve().parent
# SRBD_QP_LIB: an alternative build of the same library (A/B experiments,
# scripts/dev/ab_variants.py); default the in-tree product build
LIB_PATH = Path(os.environ.get("SRBD_QP_LIB") or (PKG_DIR / "libsrbd_qp.so"))

_dp = C.c_void_p


class SrbdQpError(RuntimeError):
    pass


class Dims(C.Structure):
    _fields_ = [("N", C.c_int), ("nx", C.c_int), ("nu", C.c_int), ("ng", C.c_int),
                ("has_box_u", C.c_int), ("has_box_x", C.c_int), ("layout", C.c_int)]


class Settings(C.Structure):
    _fields_ = [("mode", C.c_int), ("iter_max", C.c_int), ("alpha_min", C.c_double),
                ("mu0", C.c_double), ("tol_stat", C.c_double), ("tol_eq", C.c_double),
                ("tol_ineq", C.c_double), ("tol_comp", C.c_double), ("reg_prim", C.c_double),
                ("warm_start", C.c_int), ("pred_corr", C.c_int), ("ric_alg", C.c_int),
                ("split_step", C.c_int), ("compute_residuals", C.c_int),
                ("f64_rescue", C.c_int), ("f32_iters", C.c_int), ("lq_fact", C.c_int)]


DATA_FIELDS = ("A", "B", "b", "Q", "S", "R", "q", "r",
               "lbu", "ubu", "lbu_mask", "ubu_mask",
               "lbx", "ubx", "lbx_mask", "ubx_mask",
               "C", "D", "lg", "ug", "lg_mask", "ug_mask", "x0")
SOL_FIELDS = ("x", "u", "pi", "P", "p", "K", "k", "status", "iter", "res", "obj", "stat")


class Data(C.Structure):
    _fields_ = [(n, _dp) for n in DATA_FIELDS]


class Solution(C.Structure):
    _fields_ = [(n, _dp) for n in SOL_FIELDS]


# soft boxes (srbd_qp_soft_f64 / srbd_qp_slack_f64; the header's field order)
SOFT_FIELDS = ("soft_u", "soft_x", "Zl_u", "Zu_u", "zl_u", "zu_u", "Zl_x", "Zu_x", "zl_x", "zu_x",
               "lls_u", "lus_u", "lls_x", "lus_x")
SLACK_FIELDS = ("sl_u", "su_u", "sl_x", "su_x")


class Soft(C.Structure):
    _fields_ = [(n, _dp) for n in SOFT_FIELDS]


class Slack(C.Structure):
    _fields_ = [(n, _dp) for n in SLACK_FIELDS]


# the backward pass's outputs (srbd_qp_grad_f64; the header's field order): NULL = not asked for
GRAD_FIELDS = ("A", "B", "b", "Q", "S", "R", "q", "r", "x0")


class Grad(C.Structure):
    _fields_ = [(n, _dp) for n in GRAD_FIELDS]


# the gradients of the rows and bounds (srbd_qp_grad_rows_f64; the header's field order)
GRAD_ROWS_FIELDS = ("D", "lg", "ug", "lbu", "ubu")


class GradRows(C.Structure):
    _fields_ = [(n, _dp) for n in GRAD_ROWS_FIELDS]


# the linearisation's backward outputs (srbd_lin_grad_f64; the header's field order): per field the
# shape behind the batch dimension, with the horizon N
LIN_GRAD_FIELDS = ("mass", "Lbody", "mu", "Q", "Qf", "R", "x_ref", "foot_r", "foot_l", "fz_max")


class LinGrad(C.Structure):
    _fields_ = [(n, _dp) for n in LIN_GRAD_FIELDS]


def _lin_grad_shape(name, N):
    return {"mass": (), "Lbody": (3,), "mu": (), "Q": (12,), "Qf": (12,), "R": (), "x_ref": (N + 1, 12),
            "foot_r": (N, 3), "foot_l": (N, 3), "fz_max": (N, 2)}[name]


# srbd_qp_solve_host_cb_f64's callback: void (*)(void* ctx)
FACTORS_CB = C.CFUNCTYPE(None, C.c_void_p)


# fp32 twins (srbd_qp_data_f32 / srbd_qp_solution_f32): same field order
class Data32(C.Structure):
    _fields_ = [(n, _dp) for n in DATA_FIELDS]


class Solution32(C.Structure):
    _fields_ = [(n, _dp) for n in SOL_FIELDS]


MODES = {"SpeedAbs": 0, "Speed": 1, "Balance": 2, "Robust": 3}


class ModelParams(C.Structure):
    """srbd_model_params (include/srbd_qp.h): mpc_option.yaml / setupDynamics."""
    _fields_ = [("Q", C.c_double * 12), ("Qf", C.c_double * 12), ("R", C.c_double),
                ("dt", C.c_double), ("Lbody", C.c_double * 3), ("mu_b", C.c_double),
                ("theta_b", C.c_double), ("mass", C.c_double), ("foot_r", C.c_double * 3),
                ("foot_l", C.c_double * 3), ("mu", C.c_double), ("Lfx", C.c_double),
                ("Lfz", C.c_double), ("fmax", C.c_double), ("fmin", C.c_double),
                ("x_ref", C.c_double * 12), ("qf_scale", C.c_double),
                ("u_lo", C.c_double * 12), ("u_hi", C.c_double * 12)]


SRBD_CONSTRAINTS = {"none": 0, "box_u": 1, "cone": 2}


class LsParams(C.Structure):
    """srbd_linesearch_params (NMPC_solver.h:97-103)."""
    _fields_ = [(n, C.c_double) for n in ("theta_max", "theta_min", "eta", "beta_phi",
                                         "beta_theta", "beta_alpha", "alpha_min")]


def _check_tensor(name, t, dtypes, shape, device, holder="the trajectories", any_gpu=False, expected=None,
                  or_else=""):
    """ValueError unless t is a contiguous torch tensor of one of `dtypes`, of `shape`, on `device`.
    shape: per dimension an int (that size), a str (a name such as "B": any size from 1) or None
    (any size); `expected` replaces it in the message.  device: where `holder` lives; None: no
    device is asked for, or with any_gpu any GPU is."""
    import torch
    if not isinstance(t, torch.Tensor) or t.dtype not in dtypes:
        raise ValueError(f"{name} must be a {' or '.join(dict.fromkeys(str(d) for d in dtypes))} tensor{or_else}")
    fits = lambda size, want: size == want if isinstance(want, int) else (want is None or size >= 1)
    if t.dim() != len(shape) or not all(fits(s, w) for s, w in zip(t.shape, shape)):
        raise ValueError(f"{name} has shape {tuple(t.shape)}, expected {expected or tuple(shape)}")
    if not t.is_contiguous():
        raise ValueError(f"{name} must be contiguous")
    if (any_gpu and t.device.type != "cuda") or (device is not None and t.device != device):
        raise ValueError(f"{name} is on {t.device}, {holder} on {device if device is not None else 'a GPU'}")


class PlanStruct(C.Structure):
    """srbd_plan_f64: device pointers, NULL = the value in srbd_model_params."""
    _fields_ = [(n, _dp) for n in ("x_ref", "foot_r", "foot_l", "fz_max")]


class Plan:
    """Per-robot, per-stage overrides of ModelParams for srbd_linearize / srbd_linesearch /
    srbd_nmpc (srbd_plan_f64): torch fp64 device tensors, each optional.

    x_ref  [B][N+1][12]  reference state per stage (one robot's block is an Eigen
                         MatrixXd(12, N+1), the reference's x_ref_)
    foot_r [B][N][3]     right-foot position at stage k
    foot_l [B][N][3]     left-foot position
    fz_max [B][N][2]     normal-force limit (right, left): the contact schedule; a swing
                         foot gets a small positive limit

    The holder keeps the tensors alive; the calls check dtype, contiguity and shapes."""
    FIELDS = {"x_ref": (1, 12), "foot_r": (0, 3), "foot_l": (0, 3), "fz_max": (0, 2)}

    def __init__(self, x_ref=None, foot_r=None, foot_l=None, fz_max=None):
        self.x_ref, self.foot_r, self.foot_l, self.fz_max = x_ref, foot_r, foot_l, fz_max

    def struct(self, B: int, N: int, device=None) -> PlanStruct:
        """The C struct for a batch of B robots over N stages (the horizon, or the P stages of a
        rollout's long plan); ValueError on a mismatch."""
        import torch
        ps = PlanStruct()
        for name, (extra, width) in self.FIELDS.items():
            t = getattr(self, name)
            if t is None:
                continue
            _check_tensor(f"plan.{name}", t, (torch.float64,), (int(B), int(N) + extra, width), device)
            setattr(ps, name, t.data_ptr())
        return ps


def _plan_ref(plan: Optional["Plan"], B: int, N: int, device):
    """byref(PlanStruct) or None (a NULL plan) for the _plan_ entry points."""
    return None if plan is None else C.byref(plan.struct(B, N, device))


class RobotsStruct(C.Structure):
    """srbd_robots_f64: device pointers, NULL = the value in srbd_model_params."""
    _fields_ = [(n, _dp) for n in ("mass", "Lbody", "mu", "Q", "Qf", "R")]


ROBOT_ROLES = {"model": 0, "plant": 1}


class Robots:
    """Per-robot overrides of six constants of ModelParams (srbd_robots_f64) for
    Handle.set_robots: torch fp64 device tensors, each optional.

    mass [B]   Lbody [B][3]   mu [B]   Q [B][12]   Qf [B][12]   R [B]

    B is the same in every field and at least the batch of the calls that follow.  As the
    handle's "model" role all six apply; its "plant" role (the true robot that srbd_advance and
    srbd_rollout integrate) takes mass and Lbody only.  Dtype, contiguity, shapes and device
    are checked here, with ValueError, before the library sees the pointers."""
    FIELDS = {"mass": (), "Lbody": (3,), "mu": (), "Q": (12,), "Qf": (12,), "R": ()}
    PLANT_FIELDS = ("mass", "Lbody")

    def __init__(self, mass=None, Lbody=None, mu=None, Q=None, Qf=None, R=None):
        self.mass, self.Lbody, self.mu, self.Q, self.Qf, self.R = mass, Lbody, mu, Q, Qf, R

    def struct(self, role: str = "model", device=None) -> RobotsStruct:
        """The C struct for `role`; ValueError on a field the role does not take or a tensor
        that does not fit.  `device`: the handle's torch device."""
        import torch
        if role not in ROBOT_ROLES:
            raise ValueError(f"unknown robots role {role!r}, expected 'model' or 'plant'")
        rs = RobotsStruct()
        rows = None
        for name, tail in self.FIELDS.items():
            t = getattr(self, name)
            if t is None:
                continue
            if role == "plant" and name not in self.PLANT_FIELDS:
                raise ValueError(f"robots.{name}: the plant role takes mass and Lbody only")
            _check_tensor(f"robots.{name}", t, (torch.float64,), ("B",) + tail, device, "the handle", any_gpu=True)
            if rows is not None and t.shape[0] != rows:
                raise ValueError(f"robots.{name} has {t.shape[0]} rows, the other fields {rows}")
            rows = t.shape[0]
            setattr(rs, name, t.data_ptr())
        self.rows = rows
        return rs


class TerrainStruct(C.Structure):
    """srbd_terrain_f64."""
    _fields_ = [("height", _dp), ("maps", C.c_int), ("nx", C.c_int), ("ny", C.c_int), ("x0", C.c_double),
                ("y0", C.c_double), ("cell", C.c_double), ("map_r", _dp), ("search", C.c_int),
                ("w_rough", C.c_double)]


class Terrain:
    """Height maps for Handle.set_terrain (srbd_terrain_f64).  height: a torch fp64 device tensor
    [maps][ny][nx], or [ny][nx] for one map; sample (j, i) lies at (x0 + i cell, y0 + j cell) and
    the height between samples is the clamped bilinear of include/srbd_qp.h.  map_r: an int32
    device tensor [B], robot i's map (None: map 0; its values are the caller's contract).
    search (0..3): the planner picks each touchdown among the (2 search + 1)^2 cells around the
    nominal foothold, by cell^2 |d|^2 + w_rough roughness^2.  Dtype, contiguity, shapes and
    device are checked here, with ValueError; the numbers by the library."""

    def __init__(self, height, x0, y0, cell, map_r=None, search=0, w_rough=0.0):
        self.height, self.x0, self.y0, self.cell = height, x0, y0, cell
        self.map_r, self.search, self.w_rough = map_r, search, w_rough
        self.rows = None

    def struct(self, device=None) -> TerrainStruct:
        import torch
        h = self.height
        _check_tensor("terrain.height", h, (torch.float64,), (None,) * (3 if getattr(h, "ndim", 2) == 3 else 2), device,
                      "the handle", any_gpu=True, expected="[maps][ny][nx] or [ny][nx]")
        maps = h.shape[0] if h.dim() == 3 else 1
        ts = TerrainStruct(h.data_ptr() or None, int(maps), int(h.shape[-1]), int(h.shape[-2]), float(self.x0),
                           float(self.y0), float(self.cell), None, int(self.search), float(self.w_rough))
        m = self.map_r
        self.rows = None
        if m is not None:
            _check_tensor("terrain.map_r", m, (torch.int32,), ("B",), h.device, "the height", expected="(B,)")
            ts.map_r = m.data_ptr()
            self.rows = int(m.shape[0])
        return ts


class ContactStruct(C.Structure):
    """srbd_contact_f64."""
    _fields_ = [("mu", C.c_double), ("mu_r", _dp), ("Ltx", C.c_double), ("Lty", C.c_double), ("Ltz", C.c_double),
                ("fz_hi", C.c_double), ("fz_contact", C.c_double), ("ground_z", C.c_double),
                ("ground", TerrainStruct), ("z_min", C.c_double), ("cos_tilt_min", C.c_double), ("fallen", _dp),
                ("alive", _dp), ("sat", _dp)]


class Contact:
    """The plant's contact model and fall detection for Handle.set_contact (srbd_contact_f64;
    include/srbd_qp.h states the plant step with it).  mu: the true friction coefficient, or
    mu_r, a torch fp64 device tensor [B]; Lt = (Ltx, Lty, Ltz): |tau_a| <= Lt_a fz per foot; fz_hi:
    the largest normal force of a foot in contact (inf allowed); fz_contact: foot f is in contact
    iff the plan's fz_max[:, 0, f] exceeds it; ground: a Terrain, the TRUE ground under the feet
    (None: flat at ground_z, the feet keep their planned z; its search / w_rough are ignored);
    z_min, cos_tilt_min: the fall thresholds on the body's height above the true ground and on
    expm(x[0:3])[2][2].  fallen, alive: int32 device tensors [B], sat: a uint32 (or int32) device
    tensor [B]; all three optional and in/out (alive needs fallen): zero them before a rollout.
    Dtype, contiguity, shapes and device are checked here, with ValueError; the numbers by the
    library.  The holder keeps the tensors alive."""

    def __init__(self, mu=0.5, mu_r=None, Lt=(0.0, 0.05, 0.05), fz_hi=float("inf"), fz_contact=0.0, ground_z=0.0,
                 ground: Optional["Terrain"] = None, z_min=0.0, cos_tilt_min=0.0, fallen=None, alive=None,
                 sat=None):
        self.mu, self.mu_r, self.Lt, self.fz_hi, self.fz_contact = mu, mu_r, Lt, fz_hi, fz_contact
        self.ground_z, self.ground, self.z_min, self.cos_tilt_min = ground_z, ground, z_min, cos_tilt_min
        self.fallen, self.alive, self.sat = fallen, alive, sat
        self.rows = None

    def struct(self, device=None) -> ContactStruct:
        import torch
        if len(self.Lt) != 3:
            raise ValueError(f"contact.Lt needs three values (x, y, z), got {len(self.Lt)}")
        cs = ContactStruct()
        cs.mu, cs.fz_hi, cs.fz_contact = float(self.mu), float(self.fz_hi), float(self.fz_contact)
        cs.Ltx, cs.Lty, cs.Ltz = (float(v) for v in self.Lt)
        cs.ground_z, cs.z_min, cs.cos_tilt_min = float(self.ground_z), float(self.z_min), float(self.cos_tilt_min)
        rows = []
        kinds = (("mu_r", (torch.float64,)), ("fallen", (torch.int32,)), ("alive", (torch.int32,)),
                 ("sat", (getattr(torch, "uint32", torch.int32), torch.int32)))
        for name, dtypes in kinds:
            t = getattr(self, name)
            if t is None:
                continue
            _check_tensor(f"contact.{name}", t, dtypes, ("B",), device, "the handle", any_gpu=True, expected="(B,)")
            rows.append(int(t.shape[0]))
            setattr(cs, name, t.data_ptr())
        if self.alive is not None and self.fallen is None:
            raise ValueError("contact.alive needs contact.fallen")
        if self.ground is not None:
            cs.ground = self.ground.struct(device)
            if self.ground.rows is not None:
                rows.append(self.ground.rows)
        self.rows = min(rows) if rows else None
        return cs


class ActiveStruct(C.Structure):
    """srbd_active_f64."""
    _fields_ = [("mask", _dp), ("skip_fallen", C.c_int), ("compact", C.c_int)]


class Active:
    """Which robots the NMPC step steps, for Handle.set_active (srbd_active_f64; include/srbd_qp.h
    states what a robot that is not stepped keeps).  mask: an int32 device tensor [B], robot i is
    stepped iff mask[i] != 0 (None: all); skip_fallen: a robot whose contact.fallen is set when the
    step starts is not stepped (needs a Contact with fallen on the handle); compact: every SQP
    iteration is launched over the robots that still iterate only (needs warm_start = 0).  Dtype,
    contiguity, shape and device are checked here, with ValueError.  The holder keeps the tensor
    alive."""

    def __init__(self, mask=None, skip_fallen=False, compact=False):
        self.mask, self.skip_fallen, self.compact = mask, skip_fallen, compact
        self.rows = None

    def struct(self, device=None) -> ActiveStruct:
        import torch
        self.rows = None
        if self.mask is not None:
            _check_tensor("active.mask", self.mask, (torch.int32,), ("B",), device, "the handle", any_gpu=True,
                          expected="(B,)")
            self.rows = int(self.mask.shape[0])
        return ActiveStruct(_tensor_ptr(self.mask) or None, int(self.skip_fallen), int(self.compact))


class AdvanceStruct(C.Structure):
    """srbd_advance_f64."""
    _fields_ = [("substeps", C.c_int), ("wrench", _dp)]


class RolloutStruct(C.Structure):
    """srbd_rollout_f64."""
    _fields_ = [("ticks", C.c_int), ("plan_stages", C.c_int), ("substeps", C.c_int), ("wrench", _dp),
                ("alpha_reset", C.c_double), ("x_log", _dp), ("u_log", _dp), ("sqp_iter_log", _dp),
                ("converged_log", _dp)]


class PlantRolloutStruct(C.Structure):
    """srbd_plant_rollout_f64."""
    _fields_ = [("ticks", C.c_int), ("substeps", C.c_int), ("foot_stages", C.c_int), ("u", _dp), ("foot_r", _dp),
                ("foot_l", _dp), ("wrench", _dp)]


PLANT_GRAD_FIELDS = ("x0", "u", "foot_r", "foot_l", "wrench", "mass", "Lbody")


class PlantGrad(C.Structure):
    """srbd_plant_grad_f64."""
    _fields_ = [(n, _dp) for n in PLANT_GRAD_FIELDS]


def _plant_grad_shape(name, T):
    return {"x0": (12,), "u": (T, 12), "foot_r": (T, 3), "foot_l": (T, 3), "wrench": (T, 6), "mass": (),
            "Lbody": (3,)}[name]


class GaitStruct(C.Structure):
    """srbd_gait_f64."""
    _fields_ = [("period", C.c_int), ("swing", C.c_int * 2), ("offset", C.c_int * 2), ("period_r", _dp),
                ("swing_r", _dp), ("offset_r", _dp), ("hip", (C.c_double * 2) * 2), ("ground_z", C.c_double),
                ("k_raibert", C.c_double), ("fz_stance", C.c_double), ("fz_swing", C.c_double),
                ("anchor", C.c_int)]


class RolloutGaitStruct(C.Structure):
    """srbd_rollout_gait_f64."""
    _fields_ = [("cmd", _dp), ("ref_pose", _dp), ("foot_now", _dp), ("tick0", C.c_longlong),
                ("foot_log", _dp), ("fz_log", _dp)]


class Gait:
    """A gait for srbd_gait_plan / srbd_rollout_gait (srbd_gait_f64).  period, swing = (right,
    left) and offset = (right, left) are in stages: ints for every robot, or torch int32 device
    tensors [B] / [B][2] / [B][2] for per-robot gaits (the struct's _r arrays; their values are
    the caller's contract).  hip = ((x, y) right, (x, y) left): the nominal foothold relative to
    the body in the heading frame; ground_z: the foothold height; k_raibert: the velocity-error
    gain (s); fz_stance / fz_swing: fz_max of a stance / swing stage; anchor: 0 carries the
    reference position, 1 restarts it from the measured xy every tick.
    The holder keeps the tensors alive; the calls check dtype, contiguity, shapes and device."""
    INT_FIELDS = {"period": (), "swing": (2,), "offset": (2,)}

    def __init__(self, period=1, swing=(0, 0), offset=(0, 0), hip=((0.0, -0.1), (0.0, 0.1)),
                 ground_z=0.0, k_raibert=0.0, fz_stance=1000.0, fz_swing=1.0, anchor=0):
        self.period, self.swing, self.offset = period, swing, offset
        self.hip, self.ground_z, self.k_raibert = hip, ground_z, k_raibert
        self.fz_stance, self.fz_swing, self.anchor = fz_stance, fz_swing, anchor

    def struct(self, B: int, device=None) -> GaitStruct:
        """The C struct for a batch of B robots; ValueError on a tensor that does not fit."""
        import torch
        gs = GaitStruct()
        for name, tail in self.INT_FIELDS.items():
            v = getattr(self, name)
            if isinstance(v, torch.Tensor):
                _check_tensor(f"gait.{name}", v, (torch.int32,), (int(B),) + tail, device, or_else=" or Python ints")
                setattr(gs, name + "_r", v.data_ptr())
            elif tail:
                if len(v) != 2:
                    raise ValueError(f"gait.{name} needs two values (right, left), got {len(v)}")
                for f in range(2):
                    getattr(gs, name)[f] = int(v[f])
            else:
                gs.period = int(v)
        for f in range(2):
            for i in range(2):
                gs.hip[f][i] = float(self.hip[f][i])
        gs.ground_z, gs.k_raibert = float(self.ground_z), float(self.k_raibert)
        gs.fz_stance, gs.fz_swing, gs.anchor = float(self.fz_stance), float(self.fz_swing), int(self.anchor)
        return gs


def _prototypes():
    """Every function include/srbd_qp.h declares: name -> (restype, argtypes, needed).  needed =
    False marks a name that an older build, loaded through SRBD_QP_LIB for an A/B run, may lack:
    lib() skips it there, and a call to it fails with AttributeError as it always did."""
    P, i, vp = C.POINTER, C.c_int, C.c_void_p
    h, st, mp, ls, plan = vp, P(Settings), P(ModelParams), P(LsParams), P(PlanStruct)
    d64, s64, d32, s32 = P(Data), P(Solution), P(Data32), P(Solution32)
    always, maybe = True, False
    return {
        "srbd_qp_abi_version": (i, [], always),
        "srbd_qp_create": (i, [P(Dims), i, i, P(vp)], always),
        "srbd_qp_destroy": (None, [h], always),
        "srbd_qp_synchronize": (i, [h], always),
        "srbd_qp_stream": (vp, [h], always),
        "srbd_qp_workspace_bytes": (C.c_size_t, [h], always),
        "srbd_qp_memory_bytes": (C.c_size_t, [h], maybe),  # ABI 9
        "srbd_qp_default_settings": (None, [st], always),
        "srbd_qp_check_settings": (i, [st], always),
        "srbd_qp_status_string": (C.c_char_p, [i], always),
        "srbd_qp_error_string": (C.c_char_p, [i], always),
        "srbd_qp_last_error": (C.c_char_p, [], always),
        "srbd_qp_solve_f64": (i, [h, i, st, d64, s64, vp], always),
        "srbd_qp_solve_host_f64": (i, [h, i, st, d64, s64], always),
        "srbd_qp_solve_f32": (i, [h, i, st, d32, s32, vp], always),
        "srbd_qp_solve_host_f32": (i, [h, i, st, d32, s32], always),
        "srbd_qp_solve_soft_f64": (i, [h, i, st, d64, P(Soft), s64, P(Slack), vp], maybe),  # soft boxes
        "srbd_qp_solve_soft_host_f64": (i, [h, i, st, d64, P(Soft), s64, P(Slack)], maybe),
        "srbd_qp_solve_backward_f64": (i, [h, i, st, d64, s64, vp, vp, C.c_double, P(Grad), vp], maybe),  # backward
        "srbd_qp_backward_pinned_f64": (i, [h, i, vp, vp], maybe),
        "srbd_qp_solve_backward_rows_f64": (i, [h, i, st, d64, s64, vp, vp, C.c_double, C.c_double, P(Grad),
                                                P(GradRows), vp], maybe),  # general rows, bounds
        "srbd_qp_backward_active_f64": (i, [h, i, vp, vp], maybe),
        "srbd_qp_solve_host_cb_f64": (i, [h, i, st, d64, s64, FACTORS_CB, vp], maybe),  # ABI 12
        "srbd_qp_host_staging_f64": (i, [h, i, st, d64, s64], maybe),  # ABI 10
        "srbd_qp_multi_create": (i, [P(Dims), i, P(i), i, P(vp)], maybe),  # ABI 10
        "srbd_qp_multi_destroy": (None, [vp], maybe),
        "srbd_qp_multi_handle": (vp, [vp, i], maybe),
        "srbd_qp_multi_solve_f64": (i, [vp, P(i), st, d64, s64, vp, vp, vp], maybe),
        "srbd_qp_multi_solve_f32": (i, [vp, P(i), st, d32, s32, vp, vp, vp], maybe),  # ABI 11
        "srbd_qp_srbd_default_params": (None, [mp], always),
        "srbd_qp_srbd_default_linesearch": (None, [ls], always),
        "srbd_qp_srbd_linearize_f64": (i, [h, i, mp, i, vp, vp, d64, vp], always),
        "srbd_qp_srbd_linesearch_f64": (i, [h, i, mp, ls] + [vp] * 8, always),
        "srbd_qp_srbd_nmpc_f64": (i, [h, i, mp, ls, st, i, i] + [vp] * 6, always),
        "srbd_qp_srbd_linearize_plan_f64": (i, [h, i, mp, plan, i, vp, vp, d64, vp], maybe),  # plans
        "srbd_qp_srbd_linesearch_plan_f64": (i, [h, i, mp, plan, ls] + [vp] * 8, maybe),
        "srbd_qp_srbd_nmpc_plan_f64": (i, [h, i, mp, plan, ls, st, i, i] + [vp] * 6, maybe),
        "srbd_qp_srbd_advance_f64": (i, [h, i, mp, plan, P(AdvanceStruct)] + [vp] * 5, maybe),  # the closed loop
        "srbd_qp_srbd_rollout_f64": (i, [h, i, mp, plan, ls, st, i, i, P(RolloutStruct)] + [vp] * 4, maybe),
        "srbd_qp_srbd_set_robots_f64": (i, [h, i, P(RobotsStruct)], maybe),
        "srbd_qp_srbd_linearize_backward_f64": (i, [h, i, mp, plan, i, vp, vp, d64, P(LinGrad), vp], maybe),
        "srbd_qp_srbd_solve_backward_f64": (i, [h, i, st, mp, plan, i, vp, vp, d64, s64, vp, vp, C.c_double, C.c_double,
                                                P(LinGrad), vp, vp], maybe),  # the fused backward pass
        "srbd_qp_srbd_plant_rollout_f64": (i, [h, i, mp, P(PlantRolloutStruct), vp, vp, vp], maybe),  # the plant
        "srbd_qp_srbd_plant_rollout_backward_f64": (i, [h, i, mp, P(PlantRolloutStruct), vp, vp, P(PlantGrad), vp],
                                                    maybe),
        "srbd_qp_srbd_set_terrain_f64": (i, [h, P(TerrainStruct)], maybe),
        "srbd_qp_srbd_terrain_height_f64": (i, [h, i] + [vp] * 4, maybe),
        "srbd_qp_srbd_set_contact_f64": (i, [h, P(ContactStruct)], maybe),
        "srbd_qp_srbd_set_active_f64": (i, [h, P(ActiveStruct)], maybe),  # active sets
        "srbd_qp_srbd_step_work": (i, [h, P(C.c_longlong), P(C.c_longlong)], maybe),
        "srbd_qp_srbd_gait_plan_f64": (i, [h, i, mp, P(GaitStruct), vp, vp, C.c_longlong] + [vp] * 7, maybe),
        "srbd_qp_srbd_rollout_gait_f64": (i, [h, i, mp, P(GaitStruct), P(RolloutGaitStruct), ls, st, i, i,
                                              P(RolloutStruct)] + [vp] * 4, maybe),
    }


PROTOTYPES = _prototypes()
_lib = None


def lib():
    """Load libsrbd_qp.so (raises SrbdQpError if it was not built)."""
    global _lib
    if _lib is None:
        if not LIB_PATH.exists():
            raise SrbdQpError(f"{LIB_PATH} not built; run `make` (or __graft_entry__.build())")
        # torch bundles its own libamdhip64.so.7 (same soname as /opt/rocm's).
        # Load torch first so that this library binds to the HIP runtime torch
        # already uses: one runtime per process, shared device pointers/streams.
        try:
            import torch  # noqa: F401
        except ImportError:  # pragma: no cover - C-only consumers
            pass
        L = C.CDLL(str(LIB_PATH))
        for name, (restype, argtypes, needed) in PROTOTYPES.items():
            if needed or hasattr(L, name):
                f = getattr(L, name)
                f.restype, f.argtypes = restype, argtypes
        _lib = L
    return _lib


def exported_symbols():
    """Names the header declares (used by the CPU export test)."""
    hdr = (PKG_DIR.parent / "include" / "srbd_qp.h").read_text()
    import re
    return sorted(set(re.findall(r"\b(srbd_qp_[a-z0-9_]+)\s*\(", hdr)))


def check(rc: int, what: str = "srbd_qp") -> None:
    if rc != 0:
        L = lib()
        raise SrbdQpError(f"{what}: {L.srbd_qp_error_string(rc).decode()} ({rc}): "
                          f"{L.srbd_qp_last_error().decode()}")


def settings_struct(s: Optional[Dict] = None) -> Settings:
    st = Settings()
    lib().srbd_qp_default_settings(C.byref(st))
    if s:
        for k, v in s.items():
            if k == "mode":
                v = MODES[v] if isinstance(v, str) else int(v)
            if hasattr(st, k):
                setattr(st, k, v)
    return st


def status_string(code: int) -> str:
    return lib().srbd_qp_status_string(int(code)).decode()


class Handle:
    """Owns a srbd_qp_handle (device workspace + stream) for fixed dims."""

    def __init__(self, N: int, nx: int, nu: int, ng: int = 0, has_box_u: bool = False,
                 has_box_x: bool = False, capacity: int = 1, device: int = 0, layout: int = 0):
        self.dims = Dims(N, nx, nu, ng, int(has_box_u), int(has_box_x), int(layout))
        self.capacity = int(capacity)
        self.device = int(device)
        h = C.c_void_p()
        check(lib().srbd_qp_create(C.byref(self.dims), self.capacity, self.device, C.byref(h)),
              "srbd_qp_create")
        self._h = h

    @property
    def ptr(self):
        return self._h

    def stream(self) -> int:
        return int(lib().srbd_qp_stream(self._h) or 0)

    def workspace_bytes(self) -> int:
        return int(lib().srbd_qp_workspace_bytes(self._h))

    def memory_bytes(self) -> int:
        """Everything the handle holds (workspace + first-use buffers)."""
        return int(lib().srbd_qp_memory_bytes(self._h))

    def synchronize(self) -> None:
        check(lib().srbd_qp_synchronize(self._h), "srbd_qp_synchronize")

    def torch_stream(self):
        """The handle's HIP stream as a torch.cuda.ExternalStream (cached)."""
        import torch
        if getattr(self, "_ext", None) is None:
            self._ext = torch.cuda.ExternalStream(self.stream(), device=torch.device("cuda", self.device))
        return self._ext

    def solve_device(self, batch: int, settings: Settings, data, sol, stream: int = 0,
                     order: bool = True) -> None:
        """Launch on `stream` (0: the handle's own stream).  With order=True and no
        explicit stream, the launch is ordered like a torch op: after the work
        already queued on torch's current stream (which produced the inputs and
        zero-filled the outputs), and torch's stream waits for it in turn."""
        f = lib().srbd_qp_solve_f32 if isinstance(data, Data32) else lib().srbd_qp_solve_f64
        o = _order_before(self, stream, order)
        check(f(self._h, int(batch), C.byref(settings), C.byref(data), C.byref(sol),
                C.c_void_p(stream or None)), f.__name__)
        _order_after(o)

    def solve_soft_device(self, batch: int, settings: Settings, data: Data, soft: Soft, sol: Solution,
                          slack: Optional[Slack] = None, stream: int = 0, order: bool = True) -> None:
        """srbd_qp_solve_soft_f64: solve_device with soft boxes (fp64, the batched kernels);
        `slack` (optional) receives the slacks."""
        o = _order_before(self, stream, order)
        check(lib().srbd_qp_solve_soft_f64(self._h, int(batch), C.byref(settings), C.byref(data),
                                           C.byref(soft), C.byref(sol),
                                           C.byref(slack) if slack is not None else None,
                                           C.c_void_p(stream or None)), "srbd_qp_solve_soft_f64")
        _order_after(o)

    def solve_backward_device(self, batch: int, settings: Settings, data: Data, sol: Solution, gx, gu,
                              grad: Grad, act_tol: float = 0.0, stream: int = 0, order: bool = True) -> None:
        """srbd_qp_solve_backward_f64: the gradients of the QP data from the cotangents gx = dl/dx,
        gu = dl/du (torch fp64 device tensors or device addresses; either may be None = zero) at
        the forward solution in `sol`, into the non-NULL fields of `grad`.  Launched and ordered
        like solve_device, behind the forward solve on the same stream."""
        ptr = lambda t: C.c_void_p((t if isinstance(t, int) else _tensor_ptr(t)) or None)
        o = _order_before(self, stream, order)
        check(lib().srbd_qp_solve_backward_f64(self._h, int(batch), C.byref(settings), C.byref(data), C.byref(sol),
                                               ptr(gx), ptr(gu), float(act_tol), C.byref(grad),
                                               C.c_void_p(stream or None)), "srbd_qp_solve_backward_f64")
        _order_after(o)

    def backward_pinned(self, batch: int, stream: int = 0, order: bool = True):
        """srbd_qp_backward_pinned_f64: an int32 device tensor [batch], the inputs the last
        solve_backward_device on this handle (has_box_u) pinned per QP."""
        import torch
        count = torch.empty(int(batch), dtype=torch.int32, device=torch.device("cuda", self.device))
        o = _order_before(self, stream, order)
        check(lib().srbd_qp_backward_pinned_f64(self._h, int(batch), C.c_void_p(count.data_ptr()),
                                                C.c_void_p(stream or None)), "srbd_qp_backward_pinned_f64")
        _order_after(o)
        return count

    def solve_backward_rows_device(self, batch: int, settings: Settings, data: Data, sol: Solution, gx, gu,
                                   grad: Optional[Grad] = None, grad_rows: Optional[GradRows] = None,
                                   act_tol: float = 0.0, rank_tol: float = 1e-8, stream: int = 0,
                                   order: bool = True) -> None:
        """srbd_qp_solve_backward_rows_f64: solve_backward_device on a handle that may have general
        rows on the inputs (ng > 0, C = NULL), with the gradients of D, lg, ug, lbu, ubu into the
        non-NULL fields of `grad_rows`.  `grad` or `grad_rows` may be None, not both."""
        ptr = lambda t: C.c_void_p((t if isinstance(t, int) else _tensor_ptr(t)) or None)
        ref = lambda s: C.byref(s) if s is not None else None
        o = _order_before(self, stream, order)
        check(lib().srbd_qp_solve_backward_rows_f64(self._h, int(batch), C.byref(settings), C.byref(data),
                                                    C.byref(sol), ptr(gx), ptr(gu), float(act_tol), float(rank_tol),
                                                    ref(grad), ref(grad_rows), C.c_void_p(stream or None)),
              "srbd_qp_solve_backward_rows_f64")
        _order_after(o)

    def backward_active(self, batch: int, stream: int = 0, order: bool = True):
        """srbd_qp_backward_active_f64: an int32 device tensor [batch][3], what the last
        solve_backward_rows_device on this handle found per QP: inputs pinned, general rows
        accepted, general rows dropped."""
        import torch
        count = torch.empty(int(batch), 3, dtype=torch.int32, device=torch.device("cuda", self.device))
        o = _order_before(self, stream, order)
        check(lib().srbd_qp_backward_active_f64(self._h, int(batch), C.c_void_p(count.data_ptr()),
                                                C.c_void_p(stream or None)), "srbd_qp_backward_active_f64")
        _order_after(o)
        return count

    def srbd_solve_backward_device(self, batch: int, settings: Settings, params: "ModelParams", plan_ref,
                                   constraints: int, xs, us, data: Data, sol: Solution, gx, gu, grad: LinGrad,
                                   grad_x0=None, act_tol: float = 0.0, rank_tol: float = 1e-8, stream: int = 0,
                                   order: bool = True) -> None:
        """srbd_qp_srbd_solve_backward_f64: solve_backward_rows_device and the linearisation's
        backward pass in one call -- the gradients of the robots' and the plan's values into the
        non-NULL fields of `grad` and dpi[0] into grad_x0, from the cotangents gx, gu at the
        forward solution `sol` of the QP `data` that srbd_linearize wrote at xs, us.  xs, us, gx,
        gu, grad_x0: torch fp64 device tensors or device addresses; plan_ref: byref(PlanStruct) or
        None; constraints: the mode's number (SRBD_CONSTRAINTS)."""
        ptr = lambda t: C.c_void_p((t if isinstance(t, int) else _tensor_ptr(t)) or None)
        o = _order_before(self, stream, order)
        check(lib().srbd_qp_srbd_solve_backward_f64(self._h, int(batch), C.byref(settings), C.byref(params), plan_ref,
                                                    int(constraints), ptr(xs), ptr(us), C.byref(data), C.byref(sol),
                                                    ptr(gx), ptr(gu), float(act_tol), float(rank_tol), C.byref(grad),
                                                    ptr(grad_x0), C.c_void_p(stream or None)),
              "srbd_qp_srbd_solve_backward_f64")
        _order_after(o)

    def solve_soft_host(self, batch: int, settings: Settings, data: Data, soft: Soft, sol: Solution,
                        slack: Optional[Slack] = None) -> None:
        """srbd_qp_solve_soft_host_f64: host buffers, waits."""
        check(lib().srbd_qp_solve_soft_host_f64(self._h, int(batch), C.byref(settings), C.byref(data),
                                                C.byref(soft), C.byref(sol),
                                                C.byref(slack) if slack is not None else None),
              "srbd_qp_solve_soft_host_f64")

    def host_staging(self, batch: int, settings: Settings, data, sol) -> None:
        """srbd_qp_host_staging_f64: the non-NULL fields of data / sol (markers) become
        pointers into the handle's pinned staging buffer (in place)."""
        check(lib().srbd_qp_host_staging_f64(self._h, int(batch), C.byref(settings), C.byref(data),
                                             C.byref(sol)), "srbd_qp_host_staging_f64")

    def solve_host(self, batch: int, settings: Settings, data, sol, on_factors=None) -> None:
        """srbd_qp_solve_host_*; with `on_factors` (fp64), srbd_qp_solve_host_cb_f64: the
        callable runs once P, p, K, k are final in `sol`'s buffers."""
        if on_factors is not None:
            cb = FACTORS_CB(lambda _ctx: on_factors())
            check(lib().srbd_qp_solve_host_cb_f64(self._h, int(batch), C.byref(settings), C.byref(data),
                                                  C.byref(sol), cb, None), "srbd_qp_solve_host_cb_f64")
            return
        f = lib().srbd_qp_solve_host_f32 if isinstance(data, Data32) else lib().srbd_qp_solve_host_f64
        check(f(self._h, int(batch), C.byref(settings), C.byref(data), C.byref(sol)), f.__name__)

    def set_robots(self, model: Optional["Robots"] = None, plant: Optional["Robots"] = None) -> None:
        """srbd_qp_srbd_set_robots_f64 for both roles: every srbd_* call on this handle afterwards
        reads robot i's constants at row i of `model` (what the controller believes: mass, Lbody,
        mu, Q, Qf, R) and, in the plant step of srbd_advance / srbd_rollout, of `plant` (the true
        robot: mass, Lbody; a missing field is the model's).  None clears a role.  The handle
        keeps the Robots, and so their tensors, alive until they are replaced; do not modify the
        tensors while launches that read them are in flight."""
        import torch
        dev = torch.device("cuda", self.device)
        # both validated before either is set
        structs = [(role, r, None if r is None else r.struct(role, dev))
                   for role, r in (("model", model), ("plant", plant))]
        for role, r, rs in structs:
            check(lib().srbd_qp_srbd_set_robots_f64(self._h, ROBOT_ROLES[role],
                                                    None if rs is None else C.byref(rs)),
                  "srbd_qp_srbd_set_robots_f64")
        self._robots = (model, plant)

    def set_terrain(self, terrain: Optional["Terrain"] = None) -> None:
        """srbd_qp_srbd_set_terrain_f64: srbd_gait_plan and srbd_rollout_gait on this handle
        afterwards sample foothold height and reference body height from the Terrain's maps and
        select footholds on them.  None clears it: the planner without terrain, bit for bit.  The
        handle keeps the Terrain, and so its tensors, alive until it is replaced; do not modify
        them while launches that read them are in flight."""
        import torch
        ts = None if terrain is None else terrain.struct(torch.device("cuda", self.device))
        check(lib().srbd_qp_srbd_set_terrain_f64(self._h, None if ts is None else C.byref(ts)),
              "srbd_qp_srbd_set_terrain_f64")
        self._terrain = terrain

    def set_contact(self, contact: Optional["Contact"] = None) -> None:
        """srbd_qp_srbd_set_contact_f64: the plant step of srbd_advance, srbd_rollout and
        srbd_rollout_gait on this handle afterwards projects the commanded input onto what the
        feet can transmit (unilateral, the schedule's contacts, the Contact's friction and moment
        limits), stands the feet on the Contact's true ground, and records falls, survived ticks
        and the limits that were active in the Contact's tensors.  The controller never sees it.
        None clears it: the plant as it was, bit for bit.  The handle keeps the Contact, and so
        its tensors, alive until it is replaced."""
        import torch
        cs = None if contact is None else contact.struct(torch.device("cuda", self.device))
        check(lib().srbd_qp_srbd_set_contact_f64(self._h, None if cs is None else C.byref(cs)),
              "srbd_qp_srbd_set_contact_f64")
        self._contact = contact

    def set_active(self, active: Optional["Active"] = None) -> None:
        """srbd_qp_srbd_set_active_f64: srbd_nmpc, srbd_rollout and srbd_rollout_gait on this handle
        afterwards step the Active's robots only: a robot that is not stepped keeps the bits of
        xs, us and alpha and reports sqp_iter = converged = 0; with compact, every SQP iteration
        is launched over the robots that still iterate.  None (or an Active of defaults) clears
        it: the step as it was, bit for bit.  The handle keeps the Active, and so its mask, alive
        until it is replaced."""
        import torch
        a = None if active is None else active.struct(torch.device("cuda", self.device))
        check(lib().srbd_qp_srbd_set_active_f64(self._h, None if a is None else C.byref(a)),
              "srbd_qp_srbd_set_active_f64")
        self._active = active

    def step_work(self):
        """srbd_qp_srbd_step_work: (qp_solves, sqp_iterations) of the last srbd_nmpc on this handle,
        or of the last rollout summed over its ticks: the QPs passed to the solver and the SQP
        loop iterations that ran.  With Active(compact=True) qp_solves is sqp_iter.sum()."""
        q, n = C.c_longlong(0), C.c_longlong(0)
        check(lib().srbd_qp_srbd_step_work(self._h, C.byref(q), C.byref(n)), "srbd_qp_srbd_step_work")
        return int(q.value), int(n.value)

    def close(self) -> None:
        if getattr(self, "_h", None):
            lib().srbd_qp_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Multi:
    """srbd_qp_multi: one solver over several devices from one thread (a handle per
    device; shards solved concurrently, x / u / pi gathered to devices[0] by peer copies)."""

    def __init__(self, N: int, nx: int, nu: int, devices, ng: int = 0, has_box_u: bool = False,
                 has_box_x: bool = False, capacity: int = 1):
        self.dims = Dims(N, nx, nu, ng, int(has_box_u), int(has_box_x), 0)
        self.devices = list(devices)
        arr = (C.c_int * len(self.devices))(*self.devices)
        m = C.c_void_p()
        check(lib().srbd_qp_multi_create(C.byref(self.dims), int(capacity), arr, len(self.devices),
                                         C.byref(m)), "srbd_qp_multi_create")
        self._m = m

    def solve(self, batches, settings: Settings, datas, sols, root_x=None, root_u=None, root_pi=None):
        """fp64 shards (Data / Solution), or fp32 ones (Data32 / Solution32: srbd_qp_multi_solve_f32)."""
        n = len(self.devices)
        b = (C.c_int * n)(*[int(x) for x in batches])
        f32 = isinstance(datas[0], Data32)
        d = ((Data32 if f32 else Data) * n)(*datas)
        s = ((Solution32 if f32 else Solution) * n)(*sols)
        ptr = lambda t: None if t is None else C.c_void_p(t.data_ptr())
        fn = "srbd_qp_multi_solve_f32" if f32 else "srbd_qp_multi_solve_f64"
        check(getattr(lib(), fn)(self._m, b, C.byref(settings), d, s, ptr(root_x), ptr(root_u),
                                 ptr(root_pi)), fn)

    def close(self) -> None:
        if getattr(self, "_m", None):
            lib().srbd_qp_multi_destroy(self._m)
            self._m = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def _order_before(handle: "Handle", stream: int, order: bool):
    """Make the handle's stream wait for torch's current stream (inputs produced and
    outputs allocated / filled there).  No-op with an explicit stream or without an
    initialised torch CUDA context."""
    if stream or not order:
        return None
    torch = sys.modules.get("torch")
    if torch is None or not torch.cuda.is_initialized():
        return None
    ext = handle.torch_stream()
    cur = torch.cuda.current_stream(torch.device("cuda", handle.device))
    ext.wait_stream(cur)
    return cur, ext


def _order_after(o) -> None:
    """torch's current stream waits for the launch just queued on the handle's stream."""
    if o is not None:
        o[0].wait_stream(o[1])


def _tensor_ptr(t) -> int:
    return 0 if t is None else int(t.data_ptr())


def device_buffers(qp, x0: np.ndarray, device="cuda:0", want_riccati: bool = False,
                   x_init=None, u_init=None, stat_rows: int = 0, dtype=np.float64):
    """Upload an OcpQpBatch (+x0) to device tensors in the C-ABI layout.

    dtype float64 -> srbd_qp_solve_f64 structs, float32 -> the fp32 twins.
    Returns (data_tensors, sol_tensors, Data | Data32, Solution | Solution32)."""
    import torch
    np_t = np.dtype(dtype)
    p = qp.packed()
    p["x0"] = np.ascontiguousarray(x0, dtype=np.float64).reshape(qp.batch, qp.nx)
    dt = {k: (None if v is None else torch.from_numpy(np.ascontiguousarray(v, dtype=np_t)).to(device))
          for k, v in p.items()}
    nb, N, nx, nu = qp.batch, qp.N, qp.nx, qp.nu
    f64 = dict(dtype=torch.float32 if np_t == np.float32 else torch.float64, device=device)
    st = {
        "x": torch.zeros(nb, N + 1, nx, **f64) if x_init is None
        else torch.from_numpy(np.ascontiguousarray(x_init, dtype=np_t)).to(device),
        "u": torch.zeros(nb, N, nu, **f64) if u_init is None
        else torch.from_numpy(np.ascontiguousarray(u_init, dtype=np_t)).to(device),
        "pi": torch.zeros(nb, N + 1, nx, **f64),
        "status": torch.full((nb,), -1, dtype=torch.int32, device=device),
        "iter": torch.full((nb,), -1, dtype=torch.int32, device=device),
        "res": torch.zeros(nb, 4, **f64),
        "obj": torch.zeros(nb, **f64),
    }
    if stat_rows:
        st["stat"] = torch.zeros(nb, stat_rows, 18, **f64)  # HPIPM ws->stat rows
    if want_riccati:
        st["P"] = torch.zeros(nb, N + 1, nx, nx, **f64)  # col-major blocks
        st["p"] = torch.zeros(nb, N + 1, nx, **f64)
        st["K"] = torch.zeros(nb, N, nx, nu, **f64)      # col-major nu x nx blocks
        st["k"] = torch.zeros(nb, N, nu, **f64)
    DataT, SolT = (Data32, Solution32) if np_t == np.float32 else (Data, Solution)
    data = DataT(**{k: _tensor_ptr(dt.get(k)) or None for k in DATA_FIELDS})
    sol = SolT(**{k: _tensor_ptr(st.get(k)) or None for k in SOL_FIELDS})
    return dt, st, data, sol


def solve(qp, x0, settings: Optional[Dict] = None, device: str = "cuda:0", riccati: bool = False,
          x_init=None, u_init=None, handle: Optional[Handle] = None,
          stats: bool = False, dtype=np.float64) -> Dict[str, np.ndarray]:
    """Solve an OcpQpBatch on the GPU through the C-ABI; returns numpy results.

    stats=True also returns "stat" [batch][iter_max+2][18], the per-iteration
    statistics rows (alpha_aff, mu_aff, sigma, alpha_prim, alpha_dual, mu,
    res_stat, res_eq, res_ineq, res_comp, obj, 0...).

    A batch with soft boxes (qp.has_soft) goes through srbd_qp_solve_soft_f64 (fp64) and
    also returns the slacks "sl_u", "su_u" [batch][N][nu] and "sl_x", "su_x" [batch][N+1][nx]."""
    import torch
    if not torch.cuda.is_available():
        raise SrbdQpError("no GPU available: libsrbd_qp has no CPU fallback")
    dev_index = torch.device(device).index or 0
    h = handle or Handle(qp.N, qp.nx, qp.nu, qp.ng, qp.has_box_u, qp.has_box_x,
                         capacity=qp.batch, device=dev_index)
    s = settings_struct(settings)
    dt, st, data, sol = device_buffers(qp, x0, device, riccati, x_init, u_init,
                                       stat_rows=(s.iter_max + 2) if stats else 0, dtype=dtype)
    if getattr(qp, "has_soft", False):
        if np.dtype(dtype) != np.float64:
            raise SrbdQpError("soft boxes are solved in fp64 only")
        sk = {"sl_u": torch.zeros_like(st["u"]), "su_u": torch.zeros_like(st["u"]),
              "sl_x": torch.zeros_like(st["pi"]), "su_x": torch.zeros_like(st["pi"])}
        soft = Soft(**{k: _tensor_ptr(dt.get(k)) or None for k in SOFT_FIELDS})
        slack = Slack(**{k: _tensor_ptr(v) for k, v in sk.items()})
        h.solve_soft_device(qp.batch, s, data, soft, sol, slack)
        st = dict(st, **sk)
    else:
        h.solve_device(qp.batch, s, data, sol)
    h.synchronize()
    out = {k: v.cpu().numpy() for k, v in st.items()}
    if riccati:
        out["P"] = np.swapaxes(out["P"], -1, -2)
        out["K"] = np.swapaxes(out["K"], -1, -2)
    if handle is None:
        h.close()
    return out


def default_model_params() -> ModelParams:
    p = ModelParams()
    lib().srbd_qp_srbd_default_params(C.byref(p))
    return p


def model_params(p) -> ModelParams:
    """srbd_model_params from a srbd_model.SrbdParams (e.g. load_mpc_option's), on top
    of the library defaults (box limits, qf_scale = N)."""
    m = default_model_params()
    for name in ("Q", "Qf", "Lbody", "foot_r", "foot_l", "x_ref"):
        arr = getattr(m, name)
        for i, v in enumerate(getattr(p, name)):
            arr[i] = float(v)
    for name in ("R", "dt", "mu_b", "theta_b", "mass", "mu", "Lfx", "Lfz", "fmax", "fmin"):
        setattr(m, name, float(getattr(p, name)))
    return m


_TOO_FEW_ROWS = {"robots": "the handle's robots have {} rows", "terrain": "the handle's terrain has a map_r of {} rows",
                 "contact": "the handle's contact has tensors of {} rows",
                 "active": "the handle's active set has a mask of {} rows"}


def _check_rows(handle, B, *holders) -> None:
    """The call reads (a contact: also writes) rows 0..B-1 of what the handle holds from
    Handle.set_robots / set_terrain / set_contact / set_active, those named in `holders`:
    ValueError if one has fewer rows.  An active set with skip_fallen reads the contact's."""
    act = getattr(handle, "_active", None)
    if "active" in holders and "contact" not in holders and act is not None and act.skip_fallen:
        holders += ("contact",)
    for kind in holders:
        held = getattr(handle, "_" + kind, None)
        for one in held if isinstance(held, tuple) else (held,):
            if one is not None and one.rows is not None and one.rows < int(B):
                raise ValueError(_TOO_FEW_ROWS[kind].format(one.rows) + f", the batch {int(B)}")


def _call_with_plan(stem, handle, B, p, plan_ref, *tail) -> None:
    """srbd_qp_srbd_<stem>_f64, or its _plan_ twin when a plan is given."""
    name = f"srbd_qp_srbd_{stem}_f64" if plan_ref is None else f"srbd_qp_srbd_{stem}_plan_f64"
    head = (handle.ptr, int(B), C.byref(p)) + (() if plan_ref is None else (plan_ref,))
    check(getattr(lib(), name)(*head, *tail), name)


def srbd_linearize(handle: Handle, xs, us, constraints: str = "none",
                   params: Optional[ModelParams] = None, stream: int = 0, out=None,
                   plan: Optional[Plan] = None):
    """Device-side prepareQpStructures: linearise SRBD trajectories xs [B][N+1][12],
    us [B][N][12] (torch fp64 device tensors) into the solver's input buffers.
    Asynchronous on the handle's stream: keep xs / us alive (and do not reuse
    their memory from another stream) until that stream has finished.
    `plan` (a Plan) overrides the reference, the feet and the force limits per robot and
    stage; its tensors must stay alive like xs / us.  `out`: the dict a previous call returned,
    to write into (no allocation).
    Returns (dict of device tensors in the C-ABI layout, Data)."""
    import torch
    B, N1, _ = xs.shape
    N = N1 - 1
    plan_ref = _plan_ref(plan, B, N, xs.device)
    _check_rows(handle, B, "robots")
    t = out
    if t is None:
        rows = {"A": (N, 144), "B": (N, 144), "b": (N, 12), "Q": (N + 1, 144), "S": (N, 144), "R": (N, 144),
                "q": (N + 1, 12), "r": (N, 12)}
        if constraints == "box_u":
            rows.update(lbu=(N, 12), ubu=(N, 12))
        elif constraints == "cone":
            rows.update(D=(N, 24 * 12), lg=(N + 1, 24), ug=(N + 1, 24), lg_mask=(N + 1, 24), ug_mask=(N + 1, 24))
        t = {k: torch.empty(B, *shape, dtype=torch.float64, device=xs.device) for k, shape in rows.items()}
    data = Data(**{k: _tensor_ptr(t.get(k)) or None for k in DATA_FIELDS})
    p = params or default_model_params()
    o = _order_before(handle, stream, True)
    _call_with_plan("linearize", handle, B, p, plan_ref, SRBD_CONSTRAINTS[constraints], C.c_void_p(xs.data_ptr()),
                    C.c_void_p(us.data_ptr()), C.byref(data), C.c_void_p(stream or None))
    _order_after(o)
    return t, data


# the cotangents srbd_linearize_backward reads, with the shape behind the batch dimension
def _lin_cot_shapes(N, constraints):
    shapes = {"A": (N, 144), "B": (N, 144), "b": (N, 12), "Q": (N + 1, 144), "R": (N, 144), "q": (N + 1, 12),
              "r": (N, 12)}
    if constraints == "box_u":
        shapes["ubu"] = (N, 12)
    elif constraints == "cone":
        shapes.update(D=(N, 288), lg=(N + 1, 24))
    return shapes


def srbd_linearize_backward(handle: Handle, xs, us, cot: Dict, constraints: str = "none",
                            params: Optional[ModelParams] = None, plan: Optional[Plan] = None,
                            want=LIN_GRAD_FIELDS, stream: int = 0, out=None):
    """srbd_qp_srbd_linearize_backward_f64: the gradients of the handle's MODEL robots' values (mass,
    Lbody, mu, Q, Qf, R: per robot) and of the plan's (x_ref, foot_r, foot_l, fz_max: per robot and
    stage) from the cotangents `cot` of the arrays srbd_linearize writes at the same xs, us,
    constraints, params and plan -- what diff.solve_qp's backward pass returns.
    cot: {name: tensor} for any of A, B, b, Q, R, q, r (box_u: ubu; cone: D, lg), torch fp64 device
    tensors with the element counts of srbd_linearize's outputs (a matrix block may be flat or
    [..][12][12]); a missing or None entry is zero, other names are ignored.
    want: the outputs to form (LIN_GRAD_FIELDS); `out`: {name: tensor} to write into instead of
    allocating.  A gradient is per robot whether or not the handle has robots / the call a plan.
    Asynchronous on the handle's stream: keep the tensors alive like srbd_linearize's.
    Returns {name: tensor}: mass, mu, R [B], Lbody [B][3], Q, Qf [B][12], x_ref [B][N+1][12],
    foot_r, foot_l [B][N][3], fz_max [B][N][2]."""
    import torch
    if constraints not in SRBD_CONSTRAINTS:
        raise ValueError(f"unknown constraints {constraints!r}")
    _check_tensor("xs", xs, (torch.float64,), ("B", None, 12), None, any_gpu=True)
    B, N = xs.shape[0], xs.shape[1] - 1
    _check_tensor("us", us, (torch.float64,), (B, N, 12), xs.device)
    want = tuple(want)
    unknown = [n for n in want if n not in LIN_GRAD_FIELDS]
    if unknown or not want:
        raise ValueError(f"want must name outputs among {LIN_GRAD_FIELDS}, got {want}")
    plan_ref = _plan_ref(plan, B, N, xs.device)
    _check_rows(handle, B, "robots")
    ptrs = {}
    for name, shape in _lin_cot_shapes(N, constraints).items():
        t = cot.get(name)
        if t is None:
            continue
        # dtype, contiguity and device by the usual check; a matrix block may be flat or [12][rows]
        dims = t.dim() if isinstance(t, torch.Tensor) else 0
        _check_tensor(f"cot[{name!r}]", t, (torch.float64,), (B, shape[0]) + (None,) * max(dims - 2, 0), xs.device,
                      expected=(B,) + shape)
        if t.numel() != B * shape[0] * shape[1]:
            raise ValueError(f"cot[{name!r}] has shape {tuple(t.shape)}, expected {(B,) + shape}")
        ptrs[name] = t.data_ptr()
    res = {}
    for name in want:
        shape = (B,) + _lin_grad_shape(name, N)
        t = None if out is None else out.get(name)
        if t is None:
            t = torch.empty(shape, dtype=torch.float64, device=xs.device)
        else:
            _check_tensor(f"out[{name!r}]", t, (torch.float64,), shape, xs.device)
        res[name] = t
    data = Data(**{k: ptrs.get(k) or None for k in DATA_FIELDS})
    grad = LinGrad(**{n: t.data_ptr() for n, t in res.items()})
    p = params or default_model_params()
    o = _order_before(handle, stream, True)
    check(lib().srbd_qp_srbd_linearize_backward_f64(handle.ptr, int(B), C.byref(p), plan_ref,
                                                    SRBD_CONSTRAINTS[constraints], C.c_void_p(xs.data_ptr()),
                                                    C.c_void_p(us.data_ptr()), C.byref(data), C.byref(grad),
                                                    C.c_void_p(stream or None)),
          "srbd_qp_srbd_linearize_backward_f64")
    _order_after(o)
    return res


def srbd_solve_backward(handle: Handle, xs, us, data: Data, sol: Solution, gx, gu, constraints: str = "none",
                        params: Optional[ModelParams] = None, plan: Optional[Plan] = None, act_tol: float = 0.0,
                        rank_tol: float = 1e-8, want=LIN_GRAD_FIELDS, settings=None, want_x0: bool = False,
                        stream: int = 0, out=None):
    """srbd_qp_srbd_solve_backward_f64: srbd_linearize_backward's gradients straight from the solve --
    what Handle.solve_backward_rows_device followed by srbd_linearize_backward returns, without the
    gradients of the QP arrays in between.
    data: the Data srbd_linearize returned at the same xs, us, constraints, params and plan (with
    x0 set); sol: a Solution with the forward x, u, pi of the handle's solve of it; gx [B][N+1][12],
    gu [B][N][12]: the cotangents (torch fp64 device tensors; either may be None = zero).  The
    tensors behind data and sol stay the caller's to keep alive.
    want: the outputs to form (LIN_GRAD_FIELDS; may be empty with want_x0); want_x0: also "x0"
    [B][12], the gradient of the initial state; `out`: {name: tensor} to write into instead of
    allocating.  settings: as for the forward solve (reg_prim and ric_alg are read).
    Returns {name: tensor} in srbd_linearize_backward's shapes."""
    import torch
    if constraints not in SRBD_CONSTRAINTS:
        raise ValueError(f"unknown constraints {constraints!r}")
    _check_tensor("xs", xs, (torch.float64,), ("B", None, 12), None, any_gpu=True)
    B, N = xs.shape[0], xs.shape[1] - 1
    _check_tensor("us", us, (torch.float64,), (B, N, 12), xs.device)
    for name, t, rows in (("gx", gx, N + 1), ("gu", gu, N)):
        if t is not None:
            _check_tensor(name, t, (torch.float64,), (B, rows, 12), xs.device)
    want = tuple(want)
    unknown = [n for n in want if n not in LIN_GRAD_FIELDS]
    if unknown or not (want or want_x0):
        raise ValueError(f"want must name outputs among {LIN_GRAD_FIELDS}, got {want}")
    plan_ref = _plan_ref(plan, B, N, xs.device)
    _check_rows(handle, B, "robots")
    res = {}
    for name in want + (("x0",) if want_x0 else ()):
        shape = (B,) + ((12,) if name == "x0" else _lin_grad_shape(name, N))
        t = None if out is None else out.get(name)
        if t is None:
            t = torch.empty(shape, dtype=torch.float64, device=xs.device)
        else:
            _check_tensor(f"out[{name!r}]", t, (torch.float64,), shape, xs.device)
        res[name] = t
    grad = LinGrad(**{n: res[n].data_ptr() for n in want})
    st = settings if isinstance(settings, Settings) else settings_struct(settings)
    handle.srbd_solve_backward_device(B, st, params or default_model_params(), plan_ref, SRBD_CONSTRAINTS[constraints],
                                      xs, us, data, sol, gx, gu, grad, res.get("x0"), act_tol=act_tol,
                                      rank_tol=rank_tol, stream=stream)
    return res


def default_linesearch() -> LsParams:
    p = LsParams()
    lib().srbd_qp_srbd_default_linesearch(C.byref(p))
    return p


def srbd_linesearch(handle: Handle, xs, us, dx, du, alpha, params: Optional[ModelParams] = None,
                    ls: Optional[LsParams] = None, stream: int = 0, plan: Optional[Plan] = None):
    """Device filter line search (NMPCSolver::linearSearch) on a batch: xs/us
    (torch fp64, in place), dx/du the QP step, alpha [B] in/out.  Returns
    (merit [B,3] = phi, theta, dphi; converged [B]) device tensors.  `plan`: as in
    srbd_linearize."""
    import torch
    B = xs.shape[0]
    plan_ref = _plan_ref(plan, B, us.shape[1], xs.device)
    _check_rows(handle, B, "robots")
    merit = torch.empty(B, 3, dtype=torch.float64, device=xs.device)
    conv = torch.empty(B, dtype=torch.int32, device=xs.device)
    p = params or default_model_params()
    lp = ls or default_linesearch()
    ptr = lambda t: C.c_void_p(t.data_ptr())
    o = _order_before(handle, stream, True)
    _call_with_plan("linesearch", handle, B, p, plan_ref, C.byref(lp), ptr(xs), ptr(us), ptr(dx), ptr(du),
                    ptr(alpha), ptr(merit), ptr(conv), C.c_void_p(stream or None))
    _order_after(o)
    return merit, conv


def srbd_nmpc(handle: Handle, xs, us, x0, alpha, constraints: str = "none",
              settings: Optional[Dict] = None, sqp_max_loop: int = 15,
              params: Optional[ModelParams] = None, ls: Optional[LsParams] = None,
              plan: Optional[Plan] = None):
    """The SQP loop of NMPCSolver::controlLoop (NMPC_solver.cpp:362-372) for a batch
    of robots on the device (srbd_qp_srbd_nmpc_f64): xs [B][N+1][12], us [B][N][12]
    (torch fp64, updated in place), x0 [B][12], alpha [B] (in place, the persistent
    alpha_ of NMPC_solver.h:104).  Returns (sqp_iter [B], converged [B]) int32
    device tensors.  Synchronous.  `plan` (a Plan): each robot's reference trajectory,
    footstep plan and contact schedule over the horizon (srbd_qp_srbd_nmpc_plan_f64)."""
    import torch
    B = xs.shape[0]
    plan_ref = _plan_ref(plan, B, us.shape[1], xs.device)
    _check_rows(handle, B, "robots", "active")
    it = torch.zeros(B, dtype=torch.int32, device=xs.device)
    conv = torch.zeros(B, dtype=torch.int32, device=xs.device)
    p = params or default_model_params()
    lp = ls or default_linesearch()
    s = settings_struct(settings)
    ptr = lambda t: C.c_void_p(t.data_ptr())
    o = _order_before(handle, 0, True)
    _call_with_plan("nmpc", handle, B, p, plan_ref, C.byref(lp), C.byref(s), SRBD_CONSTRAINTS[constraints],
                    int(sqp_max_loop), ptr(xs), ptr(us), ptr(x0), ptr(alpha), ptr(it), ptr(conv))
    _order_after(o)
    return it, conv


def _check_f64(name, t, shape, device):
    import torch
    _check_tensor(name, t, (torch.float64,), tuple(int(n) for n in shape), device)


def srbd_advance(handle: Handle, xs, us, x=None, plan: Optional[Plan] = None, wrench=None,
                 substeps: int = 1, params: Optional[ModelParams] = None, stream: int = 0):
    """One control tick between two NMPC steps (srbd_qp_srbd_advance_f64): the applied input
    u0 = us[:, 0]; the plant state x [B][12] (in place; None: shift only) moved by `substeps` RK4
    steps of dt / substeps with u0, stage 0's feet of `plan` (this tick's window) and the
    external wrench [B][6] (torque, force; None: none); xs [B][N+1][12], us [B][N][12] shifted
    by one stage in place, the new last stage one model step from the old one.  Asynchronous on
    the handle's stream, ordered like a torch op.  Returns u0 [B][12] (a device tensor).  With a
    contact on the handle (Handle.set_contact) and a plant state, the plant applies the
    projection of u0 and the returned tensor holds that: what was really applied."""
    import torch
    B, N = us.shape[0], us.shape[1]
    dev = xs.device
    _check_f64("xs", xs, (B, N + 1, 12), dev)
    _check_f64("us", us, (B, N, 12), dev)
    if x is not None:
        _check_f64("x", x, (B, 12), dev)
    if wrench is not None:
        _check_f64("wrench", wrench, (B, 6), dev)
    plan_ref = _plan_ref(plan, B, N, dev)
    _check_rows(handle, B, "robots", "contact")
    u0 = torch.empty(B, 12, dtype=torch.float64, device=dev)
    adv = AdvanceStruct(int(substeps), _tensor_ptr(wrench) or None)
    p = params or default_model_params()
    ptr = lambda t: C.c_void_p(_tensor_ptr(t) or None)
    o = _order_before(handle, stream, True)
    check(lib().srbd_qp_srbd_advance_f64(handle.ptr, int(B), C.byref(p), plan_ref, C.byref(adv), ptr(xs),
                                         ptr(us), ptr(x), ptr(u0), C.c_void_p(stream or None)),
          "srbd_qp_srbd_advance_f64")
    _order_after(o)
    return u0


def _plant_roll(x0, u, foot_r, foot_l, wrench, substeps):
    """The tensor checks srbd_plant_rollout and its backward call share: (B, T, PlantRolloutStruct).
    x0 [B][12] names the device; u [B][T][12]; foot_r / foot_l [B][P][3] with one P >= T; wrench [B][T][6]."""
    import torch
    _check_tensor("x0", x0, (torch.float64,), ("B", 12), None, any_gpu=True)
    B, dev = x0.shape[0], x0.device
    _check_tensor("u", u, (torch.float64,), (B, None, 12), dev)
    T = u.shape[1]
    P = 0
    for name, f in (("foot_r", foot_r), ("foot_l", foot_l)):
        if f is None:
            continue
        _check_tensor(name, f, (torch.float64,), (B, None, 3), dev)
        if f.shape[1] < T or (P and f.shape[1] != P):
            raise ValueError(f"{name} has {f.shape[1]} rows per robot, expected "
                             + (f"{P}, as the other foot" if P else f"at least the {T} ticks"))
        P = f.shape[1]
    if wrench is not None:
        _check_f64("wrench", wrench, (B, T, 6), dev)
    roll = PlantRolloutStruct(T, int(substeps), P, u.data_ptr() or None, _tensor_ptr(foot_r) or None,
                              _tensor_ptr(foot_l) or None, _tensor_ptr(wrench) or None)
    return B, T, roll


def srbd_plant_rollout(handle: Handle, x0, u, foot_r=None, foot_l=None, wrench=None, substeps: int = 1,
                       params: Optional[ModelParams] = None, stream: int = 0, out=None):
    """The open-loop plant rollout (srbd_qp_srbd_plant_rollout_f64): x_traj [B][T+1][12] with
    x_traj[:, 0] = x0 [B][12] and x_traj[:, t+1] the plant state after tick t -- `substeps` RK4 steps
    of dt / substeps with the input u[:, t] (u [B][T][12], e.g. a rollout's u_log), the feet of row
    t of foot_r / foot_l [B][P][3] (P >= T; None: params') and wrench[:, t] (wrench [B][T][6]; None:
    none).  Mass and inertia are the handle's PLANT role's, else its MODEL role's, else params'.
    The handle's contact, terrain and active set are not read.  Torch fp64 device tensors, 16-byte
    aligned (x0, u, out); `out`: a tensor to write into.  Asynchronous on the handle's stream,
    ordered like a torch op."""
    import torch
    B, T, roll = _plant_roll(x0, u, foot_r, foot_l, wrench, substeps)
    _check_rows(handle, B, "robots")
    if out is None:
        out = torch.empty(B, T + 1, 12, dtype=torch.float64, device=x0.device)
    else:
        _check_f64("out", out, (B, T + 1, 12), x0.device)
    p = params or default_model_params()
    o = _order_before(handle, stream, True)
    check(lib().srbd_qp_srbd_plant_rollout_f64(handle.ptr, int(B), C.byref(p), C.byref(roll),
                                               C.c_void_p(x0.data_ptr()), C.c_void_p(out.data_ptr()),
                                               C.c_void_p(stream or None)), "srbd_qp_srbd_plant_rollout_f64")
    _order_after(o)
    return out


def srbd_plant_rollout_backward(handle: Handle, x0, u, foot_r=None, foot_l=None, wrench=None, substeps: int = 1,
                                params: Optional[ModelParams] = None, *, x_traj, gx, want=PLANT_GRAD_FIELDS,
                                stream: int = 0, out=None):
    """The adjoint of srbd_plant_rollout (srbd_qp_srbd_plant_rollout_backward_f64) at the same
    arguments: x_traj what it returned, gx [B][T+1][12] the cotangent of x_traj (row 0 included).
    want: the outputs to form (PLANT_GRAD_FIELDS); `out`: {name: tensor} to write into instead of
    allocating.  mass and Lbody are per robot whether or not a role supplies the value.
    Returns {name: tensor}: x0 [B][12], u [B][T][12], foot_r, foot_l [B][T][3], wrench [B][T][6],
    mass [B], Lbody [B][3].  Asynchronous on the handle's stream, ordered like a torch op."""
    import torch
    B, T, roll = _plant_roll(x0, u, foot_r, foot_l, wrench, substeps)
    dev = x0.device
    _check_f64("x_traj", x_traj, (B, T + 1, 12), dev)
    _check_f64("gx", gx, (B, T + 1, 12), dev)
    want = tuple(want)
    unknown = [n for n in want if n not in PLANT_GRAD_FIELDS]
    if unknown or not want:
        raise ValueError(f"want must name outputs among {PLANT_GRAD_FIELDS}, got {want}")
    _check_rows(handle, B, "robots")
    res = {}
    for name in want:
        shape = (B,) + _plant_grad_shape(name, T)
        t = None if out is None else out.get(name)
        if t is None:
            t = torch.empty(shape, dtype=torch.float64, device=dev)
        else:
            _check_tensor(f"out[{name!r}]", t, (torch.float64,), shape, dev)
        res[name] = t
    grad = PlantGrad(**{n: t.data_ptr() or None for n, t in res.items()})
    p = params or default_model_params()
    o = _order_before(handle, stream, True)
    check(lib().srbd_qp_srbd_plant_rollout_backward_f64(handle.ptr, int(B), C.byref(p), C.byref(roll),
                                                        C.c_void_p(x_traj.data_ptr()), C.c_void_p(gx.data_ptr()),
                                                        C.byref(grad), C.c_void_p(stream or None)),
          "srbd_qp_srbd_plant_rollout_backward_f64")
    _order_after(o)
    return res


def _rollout_logs(B, T, plan_stages, dev, wrench, substeps, alpha_reset):
    """((x_log, u_log, sqp_iter_log, converged_log) of a rollout of T ticks, zeroed; the
    RolloutStruct that points at them)."""
    import torch
    rows = max(T, 0)
    x_log = torch.zeros(B, rows + 1, 12, dtype=torch.float64, device=dev)
    u_log = torch.zeros(B, rows, 12, dtype=torch.float64, device=dev)
    it_log = torch.zeros(B, rows, dtype=torch.int32, device=dev)
    cv_log = torch.zeros(B, rows, dtype=torch.int32, device=dev)
    roll = RolloutStruct(T, int(plan_stages), int(substeps), _tensor_ptr(wrench) or None, float(alpha_reset),
                         x_log.data_ptr(), u_log.data_ptr() or None, it_log.data_ptr() or None,
                         cv_log.data_ptr() or None)
    return (x_log, u_log, it_log, cv_log), roll


def srbd_rollout(handle: Handle, xs, us, x, alpha, ticks: int, constraints: str = "none",
                 settings: Optional[Dict] = None, sqp_max_loop: int = 15, plan: Optional[Plan] = None,
                 plan_stages: Optional[int] = None, wrench=None, substeps: int = 1,
                 alpha_reset: float = 0.0, params: Optional[ModelParams] = None,
                 ls: Optional[LsParams] = None):
    """`ticks` ticks of the closed receding-horizon loop on the device
    (srbd_qp_srbd_rollout_f64): per tick the NMPC step (srbd_nmpc) from the plant state x with
    the plan's window of that tick, then srbd_advance with wrench[:, t].  xs [B][N+1][12],
    us [B][N][12], x [B][12], alpha [B]: torch fp64 device tensors, updated in place.
    `plan`: a Plan over plan_stages = P >= N + ticks - 1 stages (x_ref [B][P+1][12], feet
    [B][P][3], fz_max [B][P][2]); plan_stages defaults to N + ticks - 1.  wrench [B][ticks][6].
    alpha_reset > 0 starts every tick's line search from that alpha; 0 keeps the reference's
    persistent alpha_.  Synchronous.  Returns (x_log [B][ticks+1][12], u_log [B][ticks][12],
    sqp_iter_log [B][ticks], converged_log [B][ticks]) device tensors."""
    B, N, T = us.shape[0], us.shape[1], int(ticks)
    dev = xs.device
    _check_f64("xs", xs, (B, N + 1, 12), dev)
    _check_f64("us", us, (B, N, 12), dev)
    _check_f64("x", x, (B, 12), dev)
    _check_f64("alpha", alpha, (B,), dev)
    if wrench is not None:
        _check_f64("wrench", wrench, (B, max(T, 0), 6), dev)
    P = N + T - 1 if plan_stages is None else int(plan_stages)
    plan_ref = _plan_ref(plan, B, P, dev)
    _check_rows(handle, B, "robots", "contact", "active")
    logs, roll = _rollout_logs(B, T, P, dev, wrench, substeps, alpha_reset)
    p = params or default_model_params()
    lp = ls or default_linesearch()
    s = settings_struct(settings)
    ptr = lambda t: C.c_void_p(t.data_ptr())
    o = _order_before(handle, 0, True)
    check(lib().srbd_qp_srbd_rollout_f64(handle.ptr, int(B), C.byref(p), plan_ref, C.byref(lp), C.byref(s),
                                         SRBD_CONSTRAINTS[constraints], int(sqp_max_loop), C.byref(roll),
                                         ptr(xs), ptr(us), ptr(x), ptr(alpha)),
          "srbd_qp_srbd_rollout_f64")
    _order_after(o)
    return logs


def _check_gait_state(B, dev, x, ref_pose, foot_now):
    _check_f64("x", x, (B, 12), dev)
    _check_f64("ref_pose", ref_pose, (B, 3), dev)
    _check_f64("foot_now", foot_now, (B, 2, 3), dev)


def srbd_gait_plan(handle: Handle, gait: Gait, cmd, x, tick: int, ref_pose, foot_now,
                   params: Optional[ModelParams] = None, stream: int = 0, out: Optional[Plan] = None) -> Plan:
    """One tick's planning step on the device (srbd_qp_srbd_gait_plan_f64): from the command
    cmd [B][4] (vx, vy in the heading frame, wz, body height), the measured state x [B][12] and
    `tick`, the plan window of the handle's horizon N under `gait` (a Gait), with Raibert
    foothold feedback.  ref_pose [B][3] (px, py, yaw) and foot_now [B][2][3] are carried from
    tick to tick and updated in place: call once per tick.  Torch fp64 device tensors.
    Asynchronous on the handle's stream, ordered like a torch op.  Returns the window as a Plan
    (x_ref [B][N+1][12], foot_r / foot_l [B][N][3], fz_max [B][N][2]); `out`: a Plan from an
    earlier call to write into."""
    import torch
    if not isinstance(cmd, torch.Tensor) or cmd.dim() < 1:
        raise ValueError("cmd must be a torch.float64 tensor")
    B, dev = cmd.shape[0], cmd.device
    _check_f64("cmd", cmd, (B, 4), dev)
    _check_gait_state(B, dev, x, ref_pose, foot_now)
    gs = gait.struct(B, dev)
    N = handle.dims.N
    if out is None:
        f = dict(dtype=torch.float64, device=dev)
        out = Plan(torch.empty(B, N + 1, 12, **f), torch.empty(B, N, 3, **f), torch.empty(B, N, 3, **f),
                   torch.empty(B, N, 2, **f))
    elif None in (out.x_ref, out.foot_r, out.foot_l, out.fz_max):
        raise ValueError("out needs all four of x_ref, foot_r, foot_l, fz_max")
    out.struct(B, N, dev)  # the shapes
    _check_rows(handle, B, "robots", "terrain")
    p = params or default_model_params()
    ptr = lambda t: C.c_void_p(t.data_ptr())
    o = _order_before(handle, stream, True)
    check(lib().srbd_qp_srbd_gait_plan_f64(handle.ptr, int(B), C.byref(p), C.byref(gs), ptr(cmd), ptr(x),
                                           int(tick), ptr(ref_pose), ptr(foot_now), ptr(out.x_ref),
                                           ptr(out.foot_r), ptr(out.foot_l), ptr(out.fz_max),
                                           C.c_void_p(stream or None)), "srbd_qp_srbd_gait_plan_f64")
    _order_after(o)
    return out


def srbd_rollout_gait(handle: Handle, gait: Gait, cmd, xs, us, x, alpha, ref_pose, foot_now, ticks: int,
                      tick0: int = 0, constraints: str = "none", settings: Optional[Dict] = None,
                      sqp_max_loop: int = 15, wrench=None, substeps: int = 1, alpha_reset: float = 0.0,
                      params: Optional[ModelParams] = None, ls: Optional[LsParams] = None):
    """srbd_rollout that replans every tick (srbd_qp_srbd_rollout_gait_f64): per tick
    srbd_gait_plan with cmd[:, t], the current x and tick0 + t, then the NMPC step on that
    window, then srbd_advance with it and wrench[:, t].  cmd [B][ticks][4]; ref_pose [B][3] and
    foot_now [B][2][3] are updated in place like xs, us, x, alpha.  Synchronous.  Returns
    (x_log [B][ticks+1][12], u_log [B][ticks][12], sqp_iter_log [B][ticks], converged_log
    [B][ticks], foot_log [B][ticks][2][3], fz_log [B][ticks][2]) device tensors; the last two
    hold row 0 of each tick's window."""
    import torch
    B, N, T = us.shape[0], us.shape[1], int(ticks)
    dev = xs.device
    rows = max(T, 0)
    _check_f64("xs", xs, (B, N + 1, 12), dev)
    _check_f64("us", us, (B, N, 12), dev)
    _check_f64("alpha", alpha, (B,), dev)
    _check_f64("cmd", cmd, (B, rows, 4), dev)
    _check_gait_state(B, dev, x, ref_pose, foot_now)
    if wrench is not None:
        _check_f64("wrench", wrench, (B, rows, 6), dev)
    gs = gait.struct(B, dev)
    _check_rows(handle, B, "robots", "terrain", "contact", "active")
    logs, roll = _rollout_logs(B, T, 0, dev, wrench, substeps, alpha_reset)
    foot_log = torch.zeros(B, rows, 2, 3, dtype=torch.float64, device=dev)
    fz_log = torch.zeros(B, rows, 2, dtype=torch.float64, device=dev)
    gio = RolloutGaitStruct(cmd.data_ptr() or None, ref_pose.data_ptr(), foot_now.data_ptr(), int(tick0),
                            foot_log.data_ptr() or None, fz_log.data_ptr() or None)
    p = params or default_model_params()
    lp = ls or default_linesearch()
    s = settings_struct(settings)
    ptr = lambda t: C.c_void_p(t.data_ptr())
    o = _order_before(handle, 0, True)
    check(lib().srbd_qp_srbd_rollout_gait_f64(handle.ptr, int(B), C.byref(p), C.byref(gs), C.byref(gio),
                                              C.byref(lp), C.byref(s), SRBD_CONSTRAINTS[constraints],
                                              int(sqp_max_loop), C.byref(roll), ptr(xs), ptr(us), ptr(x),
                                              ptr(alpha)), "srbd_qp_srbd_rollout_gait_f64")
    _order_after(o)
    return logs + (foot_log, fz_log)


def srbd_terrain_height(handle: Handle, xy, map=None, stream: int = 0):
    """The height of the handle's terrain (Handle.set_terrain) at the points xy [n][2], point i
    on map[i] (an int32 device tensor [n]; None: map 0): srbd_qp_srbd_terrain_height_f64, the
    clamped bilinear the planner samples.  Torch fp64 device tensors; asynchronous on the
    handle's stream, ordered like a torch op.  Returns out [n]."""
    import torch
    if not isinstance(xy, torch.Tensor) or xy.dim() != 2:
        raise ValueError("xy must be a torch.float64 tensor [n][2]")
    n, dev = xy.shape[0], xy.device
    _check_f64("xy", xy, (n, 2), dev)
    if map is not None:
        _check_tensor("map", map, (torch.int32,), (int(n),), dev, "xy")
    out = torch.empty(n, dtype=torch.float64, device=dev)
    o = _order_before(handle, stream, True)
    check(lib().srbd_qp_srbd_terrain_height_f64(handle.ptr, int(n), C.c_void_p(xy.data_ptr() or None),
                                                C.c_void_p(_tensor_ptr(map) or None),
                                                C.c_void_p(out.data_ptr() or None), C.c_void_p(stream or None)),
          "srbd_qp_srbd_terrain_height_f64")
    _order_after(o)
    return out
