"""NumPy restatement of `Demonstrations.labels()` (demos.py): the hindsight labels of a recorded drive, rule by rule.

    sample (t, s) is VALID when t + H * stride <= T - 1 and done[t .. t + H * stride, s] are all 0;
    row k describes tick t + k * stride:
      x, y     ego frame v1's `point` of the position then, in the pose of tick t (nav_ref.world_to_ego, kind POINTS: fp64, rounded to fp32 once);
      yaw      d = (compass_k - compass_0) / pi in fp64;  d - 2 when d > 1, d + 2 when d < -1;  rounded to fp32;
      speed    (double)velocity_k / speed_scale, rounded to fp32;
      action   the control recorded at tick t + (k + 1) * stride;
    every word clipped to [-1, 1];  the target is the one recorded at tick t, unclipped.

`labels` returns the x, y bound beside the values: ego frame v1's stated bound (nav_ref.world_to_ego's), since the device's cos and sin may
differ from NumPy's within their 4 ulp.  Every other column has no library call in it and is compared exactly."""
import numpy as np

import nav_ref as N


def labels(pose, velocity, target, control, done, *, horizon, stride, speed_scale, xy_scale):
    """pose [T, S, 3] fp64, velocity [T, S] fp32, target [T, S, 2] fp32, control [T, S, 3] fp32, done [T, S] int.  Returns
    (index int64 [n, 2], waypoints fp32 [n, H, 7], xy_bound fp64 [n, H, 2], target fp32 [n, 2]), samples in (tick, scene) order."""
    pose, velocity = np.asarray(pose, np.float64), np.asarray(velocity, np.float32)
    target, control, done = np.asarray(target, np.float32), np.asarray(control, np.float32), np.asarray(done)
    T, S = pose.shape[:2]
    H, st = int(horizon), int(stride)
    span = H * st
    index, wps, bounds, tgt = [], [], [], []
    for t in range(T - span):
        for s in range(S):
            if (done[t:t + span + 1, s] != 0).any():
                continue
            rows = np.zeros((H, 7), np.float32)
            xy, bnd = N.world_to_ego(N.POINTS, pose[t:t + span:st, s, 0:2][None], pose[t, s][None], xy_scale)      # [1, H, 2] each
            rows[:, 0:2], bnd = xy[0], bnd[0]
            for k in range(H):
                q = pose[t + k * st, s]
                d = (q[2] - pose[t, s, 2]) / np.pi
                d = d - 2.0 if d > 1.0 else (d + 2.0 if d < -1.0 else d)
                rows[k, 2] = np.float32(d)
                rows[k, 3] = np.float32(np.float64(velocity[t + k * st, s]) / float(speed_scale))
                rows[k, 4:7] = control[t + (k + 1) * st, s]
            index.append((t, s)), wps.append(np.clip(rows, -1.0, 1.0)), bounds.append(bnd), tgt.append(target[t, s])
    n = len(index)
    return (np.array(index, np.int64).reshape(n, 2), np.array(wps, np.float32).reshape(n, H, 7), np.array(bounds).reshape(n, H, 2),
            np.array(tgt, np.float32).reshape(n, 2))
