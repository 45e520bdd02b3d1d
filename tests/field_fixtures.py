"""Test infrastructure: the fields and trajectories of tests/test_gpu_field.py, built on the CPU so that tests/test_field_cpu.py can
check their margins (tests/field_ref.py: `margins`, `hinge_margin`) without a device, before any GPU run.

HAND is the hand-checkable fixture of "cost guidance v2": two scenes of a 3 x 2 field (Gy = 3, Gx = 2) with dx = dy = 2^-2 and
origin (-0.25, 0), so every node coordinate, every u, v and every product below is exact in fp32; weight 0.5.
    scene 0   [[1, 3], [2, 4], [-8, 6]]      cell 0 = rows 0..1, cell 1 = rows 1..2 (its interpolant is negative near node [2][0])
    scene 1   all zero
"""
import numpy as np
import torch

import field_ref as FR

F32 = np.float32
HAND_CELLS = np.array([[[1, 3], [2, 4], [-8, 6]], [[0, 0], [0, 0], [0, 0]]], F32)
HAND = dict(origin=(-0.25, 0.0), cell=(0.25, 0.25), weight=0.5)
_NAN = float("nan")
# (scene, x, y, J, gx, gy, active): the expected values written out by hand from the contract's lines
HAND_POINTS = [
    # on node [0][0]: u = v = 0, fu = fv = 0; a = b = 2, top = 1, bot = 2, dv = 1, C = 1, du = 2
    (0, -0.25, 0.0, 0.5, 4.0, 2.0, 1),
    # on the LAST node [2][1]: u = 1, v = 2 -> j = min(1, 0) = 0, i = min(2, 1) = 1, fu = fv = 1; a = 2, b = 14, top = 4, bot = 6,
    # dv = 2, C = 6 = cells[2][1], du = 2 + 12 = 14
    (0, 0.0, 0.5, 3.0, 28.0, 4.0, 1),
    # inside cell 0: u = 0.5, v = 0.25; a = b = 2, top = 2, bot = 3, dv = 1, C = 2.25, du = 2
    (0, -0.125, 0.0625, 1.125, 4.0, 2.0, 1),
    # inside cell 1 on its right edge: u = 1, v = 1.5 -> fu = 1, fv = 0.5; a = 2, b = 14, top = 4, bot = 6, dv = 2, C = 5, du = 8
    (0, 0.0, 0.375, 2.5, 16.0, 4.0, 1),
    # cell 1 where the interpolant is negative: fu = 0, fv = 0.5; top = 2, bot = -8, dv = -10, C = -3: inactive
    (0, -0.25, 0.375, 0.0, 0.0, 0.0, 0),
    # one ulp outside: below x_min, and above the last row
    (0, float(np.nextafter(F32(-0.25), F32(-1))), 0.125, 0.0, 0.0, 0.0, 0),
    (0, -0.125, float(np.nextafter(F32(0.5), F32(1))), 0.0, 0.0, 0.0, 0),
    # a NaN is outside
    (0, _NAN, 0.125, 0.0, 0.0, 0.0, 0),
    (0, -0.125, _NAN, 0.0, 0.0, 0.0, 0),
    # the all-zero scene: C = 0 is not > 0
    (1, -0.125, 0.125, 0.0, 0.0, 0.0, 0),
]


def hand_field():
    return FR.field(HAND_CELLS, **HAND)


def step_cells(Sn, Gy, Gx, seed):
    """[Sn, Gy, Gx] for the step tests: values in [-0.5, 1.5], mostly positive, one all-zero cell where the raster has room."""
    g = torch.Generator().manual_seed(seed)
    c = torch.rand(Sn, Gy, Gx, generator=g) * 2 - 0.5
    if Gy >= 3 and Gx >= 3:
        c[:, :2, :2] = 0.0
    return c


# the geometry of the step tests: the raster covers [-0.6, 0.6]^2 of the clamped x0's [-1, 1]^2, so some waypoints are outside
def step_geometry(Gy, Gx):
    return dict(origin=(-0.6, -0.6), cell=(1.2 / (Gx - 1), 1.2 / (Gy - 1)))


# (rows, Sn, H, D, M, P, Gy, Gx, seed): rows no multiple of four, H = 8, 33 and 64, S < rows; a field alone and beside discs and planes.
# The seeds are picked so that the margins test_field_cpu.py asserts hold
COST_CASES = [(6, 2, 8, 7, 3, 2, 3, 5, 0), (7, 1, 8, 2, 0, 0, 2, 2, 0), (5, 5, 64, 3, 0, 1, 9, 16, 0), (9, 3, 33, 4, 32, 8, 9, 16, 0)]


def _cell(G):
    """The largest 2^-k with (G - 1) * 2^-k <= 1: the raster spans [-0.5, 0.5] where G - 1 is a power of two, a little less else."""
    return 2.0 ** -((G - 2).bit_length())


def cost_case(rows, Sn, H, D, M, P, Gy, Gx, seed):
    """-> (traj [rows, H, D], discs or None, planes or None, cells [Sn, Gy, Gx], geometry kw, designated [rows, H] bool), torch CPU.
    The designated waypoints sit exactly on a node, on the last node and just outside the raster: their cell is decided by exact
    arithmetic, not by a margin."""
    g = torch.Generator().manual_seed(1000 * seed + 7 * rows + H + Gx)
    traj = torch.rand(rows, H, D, generator=g) * 2 - 1
    discs = planes = None
    if M:
        discs = torch.zeros(Sn, M, 5)
        discs[..., :2] = torch.rand(Sn, M, 2, generator=g) * 1.6 - 0.8
        discs[..., 2:4] = (torch.rand(Sn, M, 2, generator=g) - 0.5) * (0.2 / H)
        discs[..., 4] = 0.3 + 0.6 * torch.rand(Sn, M, generator=g)
        if M >= 3:
            discs[0, 1, 4], discs[-1, 2, 4] = 0.0, float("nan")
    if P:
        planes = torch.zeros(Sn, P, 3)
        planes[..., :2] = torch.rand(Sn, P, 2, generator=g) * 2 - 1
        planes[..., 2] = torch.rand(Sn, P, generator=g) - 0.3
    cells = torch.rand(Sn, Gy, Gx, generator=g) * 2 - 0.5
    # origin -0.5 and cells of 2^-k: every node coordinate and both reciprocals are exact in fp32, so "on a node" means on it
    geo = dict(origin=(-0.5, -0.5), cell=(_cell(Gx), _cell(Gy)))
    dx, dy = geo["cell"]
    designated = torch.zeros(rows, H, dtype=torch.bool)
    traj[0, 1, 0], traj[0, 1, 1] = -0.5, -0.5                                                # node [0][0]
    traj[0, 2, 0], traj[0, 2, 1] = -0.5 + (Gx - 1) * dx, -0.5 + (Gy - 1) * dy                # the last node
    traj[0, 3, 0], traj[0, 3, 1] = float(np.nextafter(F32(-0.5), F32(-1))), 0.0              # one ulp outside
    designated[0, 1:4] = True
    return traj, discs, planes, cells, geo, designated
