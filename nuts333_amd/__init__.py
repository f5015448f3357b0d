"""nuts333_amd -- CPU-only baseline harness for ToKe79/nuts333 (NUTS 3.3.3 telnet talker).

The reference has no data-parallel numeric hot path (BASELINE.json
``north_star``): the talker path therefore has no HIP kernel and no RCCL code.  The package holds
what the north star asks for -- a scratch-tree provisioner, a talker launcher, the
closed-loop load generator and the five BASELINE configurations -- plus ``device`` / ``devpath``: the broadcast's
user-space stage as a gfx950 kernel, kept to measure what the device path would cost.
"""
__all__ = ["provision", "talker", "workloads"]
