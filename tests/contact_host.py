"""TEST INFRASTRUCTURE ONLY -- the host side of the plant's contact model
(srbd_qp_srbd_set_contact_f64): the state arrays of a batch.  The plant step with a contact
robot by robot and the host closed loop with a contact are tests/rollout_host.py's
plant_step(contact=...) and closed_loop(contact=...)."""
from __future__ import annotations

import numpy as np

__all__ = ["zero_state"]


def zero_state(B, fallen=True, alive=True, sat=True):
    """The fallen / alive / sat arrays of a batch that has not started."""
    s = {}
    if fallen:
        s["fallen"] = np.zeros(B, dtype=np.int32)
    if alive:
        s["alive"] = np.zeros(B, dtype=np.int32)
    if sat:
        s["sat"] = np.zeros(B, dtype=np.uint32)
    return s
