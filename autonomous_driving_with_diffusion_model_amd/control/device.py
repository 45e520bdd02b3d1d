"""The controller on the device: waypoints -> (throttle, steer, brake) for every scene of a tick in one launch.

`DeviceController.step` is one launch of `adx_control_step` (csrc/control.hip, "control v1" of include/adx.h): what
`Controller.control_pid` + `post_process_control` (control/controller.py) do for one scene on the host, with the PID windows
of all scenes in one device buffer that every launch reads and advances.  No host decision and no synchronisation, so the
call can be a node of a captured graph (`GraphedSampler(..., controller=...)`) and a replay carries the windows on.  The host
`Controller` stays what it was: the bit-for-bit restatement of the reference, and the yardstick this one is checked against.
"""
from __future__ import annotations

import ctypes as C
from typing import Optional, Tuple

import torch

from .. import _lib as L

SOURCES = {"pid": 0, "action": 1}
POSTS = {"none": 0, "agent": 1, "interact": 2}
MAX_WINDOW = 256


class DeviceController:
    """`cfg.PID` and `cfg.CONTROL` as `Controller` reads them.  `waypoints` = W: how many waypoints of the trajectory the PID
    path looks at (the callers pass `traj[0, :4, :2]`); `post`: "none", "agent" (e2e_driving's `post_process_control`, the
    one control/controller.py has) or "interact" (interact.py's: a brake above 0.5 also zeroes the steer); `source`: "pid", or
    "action" = the callers' D > 2 path, the post-processed last three columns of the first waypoint (no PID state is touched);
    `sign_x` = -1 is the callers' `renew_traj`; `target_scale` multiplies the target as `xy_scale` does the waypoints."""

    def __init__(self, cfg, scenes: int, device, *, waypoints: int = 4, post: str = "agent", source: str = "pid",
                 sign_x: float = -1.0, target_scale: float = 1.0):
        if post not in POSTS or source not in SOURCES:
            raise ValueError(f"DeviceController: post must be one of {sorted(POSTS)} and source one of {sorted(SOURCES)}, got "
                             f"{post!r} and {source!r}")
        p, c = cfg.PID, cfg.CONTROL
        self.scenes, self.device = int(scenes), torch.device(device)
        self.waypoints, self.post, self.source = int(waypoints), post, source
        self.sign_x, self.target_scale = float(sign_x), float(target_scale)
        self.n_turn, self.n_speed = int(p.TURN_N), int(p.SPEED_N)
        self.gains = tuple(float(v) for v in (p.TURN_KP, p.TURN_KI, p.TURN_KD, p.SPEED_KP, p.SPEED_KI, p.SPEED_KD))
        self.limits = tuple(float(v) for v in (c.AIM_DIST, c.ANGLE_THRESH, c.DIST_THRESH, c.BRAKE_SPEED, c.BRAKE_RATIO,
                                               c.CLIP_DELTA, c.MAX_THROTTLE))
        if not 1 <= self.scenes <= 65535:
            raise ValueError(f"DeviceController: scenes must be 1..65535, got {self.scenes}")
        if not (1 <= self.n_turn <= MAX_WINDOW and 1 <= self.n_speed <= MAX_WINDOW):
            raise ValueError(f"DeviceController: PID.TURN_N = {self.n_turn} and PID.SPEED_N = {self.n_speed} must be 1..{MAX_WINDOW}")
        if self.waypoints < 2:
            raise ValueError(f"DeviceController: waypoints must be at least 2, got {self.waypoints}")
        if self.device.type != "cuda":
            raise L.AdxError(f"DeviceController on {self.device}: the adx kernels only run on an MI355X (the host path is Controller)")
        if self.device.index is None:                  # "cuda" names the current device; tensors say "cuda:0"
            self.device = torch.device("cuda", torch.cuda.current_device())
        self._stride = 2 + self.n_turn + self.n_speed
        # all zero = fresh windows; the size is the library's, the layout is read back only by windows()
        nbytes = L.lib().adx_control_state_bytes(self.scenes, self.n_turn, self.n_speed)
        assert nbytes == 4 * self.scenes * self._stride, (nbytes, self.scenes, self._stride)
        self.state = torch.zeros(nbytes // 4, dtype=torch.int32, device=self.device)
        self._no_velocity = None

    # ---- what a captured graph bakes in ------------------------------------------------------------------------------------
    def key(self) -> tuple:
        return (self.scenes, self.waypoints, self.post, self.source, self.sign_x, self.target_scale, self.n_turn, self.n_speed,
                self.gains, self.limits)

    def check(self, horizon: int, dim: int, has_target: bool) -> None:
        """The refusals of the launch that depend on the trajectory's shape, raised here so that a caller can ask before it
        starts a tick."""
        H, D, W = int(horizon), int(dim), self.waypoints
        if not 2 <= H <= 64 or not 1 <= D <= 16:
            raise ValueError(f"DeviceController: trajectories of [{H}, {D}] (horizon 2..64, transition dim 1..16)")
        if W > H:
            raise ValueError(f"DeviceController: waypoints = {W} is more than the horizon {H}")
        if self.source == "action":
            if D < 3:
                raise ValueError(f"DeviceController: source='action' reads the last three columns, the transition dim is {D}")
        elif not has_target and W >= H:
            raise ValueError(f"DeviceController: without a target waypoint {W} stands in for it; the horizon is {H}")

    def _cfg(self, H: int, D: int, xy_scale: float) -> L.ControlCfg:
        return L.ControlCfg(self.scenes, H, D, self.waypoints, self.n_turn, self.n_speed, SOURCES[self.source], POSTS[self.post],
                            self.sign_x, float(xy_scale), self.target_scale, *self.gains, *self.limits)

    def step(self, traj: torch.Tensor, velocity: Optional[torch.Tensor], target: Optional[torch.Tensor] = None,
             xy_scale: float = 1.0) -> torch.Tensor:
        """traj [S, H, D] in the model's own units (clamped, before xy scaling; `xy_scale` = `model.magic_num` turns them into
        the controller's), velocity [S] (may be None with source='action', which does not read it), target None or [S, 2].
        Returns control [S, 3] = (throttle, steer, brake) and advances the windows of every scene by one sample."""
        traj = L.require_gpu_f32(traj, "traj")
        if traj.dim() != 3 or traj.shape[0] != self.scenes:
            raise ValueError(f"traj must be [{self.scenes}, H, D], got {tuple(traj.shape)}")
        S, H, D = traj.shape
        self.check(H, D, target is not None)
        if velocity is None:
            if self.source != "action":
                raise ValueError("DeviceController.step: the PID source needs `velocity` [S]")
            if self._no_velocity is None:
                self._no_velocity = torch.zeros(self.scenes, dtype=torch.float32, device=self.device)
            velocity = self._no_velocity
        velocity = L.require_gpu_f32(velocity, "velocity")
        if tuple(velocity.shape) != (S,):
            raise ValueError(f"velocity must be [{S}], got {tuple(velocity.shape)}")
        if target is not None:
            target = L.require_gpu_f32(target, "target")
            if tuple(target.shape) != (S, 2):
                raise ValueError(f"target must be [{S}, 2], got {tuple(target.shape)}")
        for name, t in (("traj", traj), ("velocity", velocity), ("target", target)):
            if t is not None and t.device != self.device:
                raise ValueError(f"{name} lives on {t.device}, the controller's state on {self.device}")
        control = torch.empty((S, 3), dtype=torch.float32, device=self.device)
        cfg = self._cfg(H, D, xy_scale)
        L.check(L.lib().adx_control_step(C.byref(cfg), traj.data_ptr(), velocity.data_ptr(), L.ptr(target), self.state.data_ptr(),
                                         control.data_ptr(), L.stream_ptr(self.device)), "adx_control_step")
        return control

    def reset(self, mask: Optional[torch.Tensor] = None) -> None:
        """Fresh windows for every scene, or for the scenes where `mask` [S] (bool or uint8, on the device) is set; a launch
        on the current stream, capturable."""
        if mask is not None:
            if tuple(mask.shape) != (self.scenes,) or mask.device != self.device or mask.dtype not in (torch.bool, torch.uint8):
                raise ValueError(f"mask must be [{self.scenes}] bool or uint8 on {self.device}, got {tuple(mask.shape)} "
                                 f"{mask.dtype} on {mask.device}")
            mask = mask.contiguous().view(torch.uint8)
        L.check(L.lib().adx_control_reset(self.state.data_ptr(), self.scenes, self.n_turn, self.n_speed, L.ptr(mask),
                                          L.stream_ptr(self.device)), "adx_control_reset")

    def windows(self) -> Tuple[torch.Tensor, torch.Tensor]:
        """Host copies (turn [S, TURN_N], speed [S, SPEED_N]) of the two windows, oldest sample first.  Synchronises: for
        tests and for inspection."""
        words = self.state.cpu().view(self.scenes, self._stride)
        rings = words[:, 2:].contiguous().view(torch.float32)
        out = []
        for which, (lo, n) in enumerate(((0, self.n_turn), (self.n_turn, self.n_speed))):
            head = (words[:, which].to(torch.int64) & 0xFFFFFFFF).remainder(n)            # the next slot = the oldest sample
            order = (head[:, None] + torch.arange(n)[None, :]).remainder(n)
            out.append(torch.gather(rings[:, lo:lo + n], 1, order))
        return out[0], out[1]

    def state_snapshot(self) -> torch.Tensor:
        return self.state.clone()

    def state_restore(self, snapshot: torch.Tensor) -> None:
        if snapshot.shape != self.state.shape or snapshot.dtype != self.state.dtype:
            raise ValueError("state_restore: not a snapshot of this controller")
        self.state.copy_(snapshot)

    def __repr__(self):
        return (f"DeviceController(scenes={self.scenes}, waypoints={self.waypoints}, post={self.post!r}, source={self.source!r}, "
                f"windows=({self.n_turn}, {self.n_speed}), device={self.device})")
