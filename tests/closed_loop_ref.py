"""The closed loop (simulation.drive around a full-stack tick) composed from the fp64 restatements of its stages, one tick as a
function of the tick's state and of its K * S candidates -- the UNet is not restated, the candidates are an input.  NumPy only: no
device and no package kernel.  Nothing here restates a stage or derives a tolerance: every value, bound and clearance is the
stage's own restatement's (nav_ref, capsule_ref, guide_ref, select_ref, select_guide_ref, commit_ref, modes_ref, fallback_ref,
control_ref, vehicle_ref, drive_ref), fed as the stage's own GPU test feeds it.

    stage        reads                                                          gives
    guide        pose P_t, world W_t, xy_scale, waypoint_dt                     discs and capsules in the ego frame (float32)
    nav          P_t, the walk's state                                          target, window, motion, the new state
    select       candidates C_t (model units), target, guide                    cost, active, the selector's index
    commit       C_t, cost, the selector's index, active, motion, its state     committed index and plan, status, the new state
    modes        C_t                                                            ModeSet
    stop         the committed plan, guide, params                              the re-timed plan, first, status, stop_at
    control      the re-timed plan, velocity v_t, target, the PID windows       control u_t, the new windows
    vehicle      u_t, hold = done_{t-1}, its state                              P_{t+1}, v_{t+1}, yaw rate
    world        W_t, the vehicle's dt                                          W_{t+1}
    metrics      P_{t+1}, v_{t+1}, yaw rate, W_{t+1}, its record                the new record, done_t

A TRANSCRIPT is what a drive leaves behind: `dict(setup=Setup, ticks=[record, ...])`, a record holding NumPy copies of every
stage's inputs and outputs under the names `roll` writes below.  `roll` produces one from the restatements themselves (a drive on
the CPU); tests/test_gpu_closed_loop_ref.py records one from the device.  `replay(transcript, wiring)` evaluates every stage on
the RECORDED inputs of that stage (so a chaotic roll-out never accumulates) and compares with its recorded output: exactly where
the stage's own GPU test compares exactly, within the stage's own bound elsewhere.  `wiring` names, per stage input, which recorded
quantity feeds it; DEFAULT is `drive`'s order, and a planted defect is another choice (DEFECTS).

Decisions (an arg-min, a hinge's side, a threshold) are compared only where the restatement's own clearance says rounding cannot
flip them, by the rule the stage's own test uses; the others are DROPPED and counted, never silently.  Values are never dropped,
but for the two that ARE a decision's outcome: the steer goes with the controller's aim and to_target, the pedals with its brake.
"""
from types import SimpleNamespace

import numpy as np

import capsule_ref as CR
import commit_ref as CM
import control_ref as CT
import drive_ref as DR
import fallback_ref as FB
import guide_ref as G
import modes_ref as MO
import nav_ref as N
import select_guide_ref as SG
import select_ref as SR
import vehicle_ref as V

F32, F64 = G.F32, G.F64
E52 = 2.0 ** -52
METRICS_CLEAR = 1e-9          # tests/test_gpu_drive.py: no contact or threshold decision nearer to equality than this
DROPPABLE = ("select", "commit", "modes", "control", "metrics")


def Setup(**kw):
    """What a drive fixes once: S, K, H, D; xy_scale, waypoint_dt; route [S, G, 2] fp64, cmd [S, G], length [S] and nav =
    dict(min_distance, max_distance, R, first); weights = (w_goal, w_smooth, w_consensus, w_guide) and hard; commit = dict(radius,
    margin, ratio, max_hold, h0, shift); modes = dict(M, radius, h0); stop_params float32 [S, 2]; control = control_ref.params(...);
    vehicle = the keywords of vehicle_ref.step; metrics = drive_ref's cfg.  `cum` [S, G] is added here."""
    s = SimpleNamespace(**kw)
    s.route = np.asarray(s.route, F64)
    s.cum = np.stack([DR.cumulative(r) for r in s.route])
    s.stop_params = np.asarray(s.stop_params, F32)
    return s


# ---- the stages --------------------------------------------------------------------------------------------------------------------
def guide_stage(pose, discs_m, boxes_m, xy_scale, dt):
    """`simulation._world_guide`: EgoFrame.discs, and Capsules.from_boxes(EgoFrame.boxes(...)) with no inflation.  dict(discs,
    discs_bound, boxes, boxes_bound, slots), None where the world holds none."""
    out = dict(discs=None, discs_bound=None, boxes=None, boxes_bound=None, slots=None)
    if discs_m is not None:
        out["discs"], out["discs_bound"] = N.world_to_ego(N.DISCS, discs_m, pose, xy_scale, dt)
    if boxes_m is not None:
        out["boxes"], out["boxes_bound"] = N.world_to_ego(N.BOXES, boxes_m, pose, xy_scale, dt)
        out["slots"] = CR.from_boxes(out["boxes"], 0.0)
    return out


def slots_bound(g, got):
    """[S, N, 7]: the bound of tests/test_gpu_nav.py's test_capsules_from_device_boxes_equal_capsules_from_host_boxes_within_the_bound.
    A slot's ends are fl(c -+ fl(s * u)), s from the sizes (the same bits on both sides): the centre's bound, |s| times the
    heading's, half an ulp of the product and of the end on each side; the velocities carry the boxes' bound; the radius is exact."""
    boxes, bound, want = g["boxes"], g["boxes_bound"], g["slots"]
    half = np.abs(boxes[..., 6].astype(F64) - boxes[..., 7]) / 2
    heading = np.maximum(bound[..., 4], bound[..., 5])
    out = np.zeros(want.shape, F64)
    for end in (0, 2):
        for xy in (0, 1):
            off = np.abs(want[..., end + xy].astype(F64) - boxes[..., xy])
            out[..., end + xy] = bound[..., xy] + half * heading + np.spacing(F32(off + 1e-30)) + \
                np.spacing(np.maximum(np.abs(got[..., end + xy]), np.abs(want[..., end + xy])))
    out[..., 4:6] = bound[..., 2:4]
    return out


def nav_stage(setup, pose, words):
    """nav_ref.nav_step from the int32 [S, 8] state words (head, valid, the previous pose as three doubles)."""
    w = np.ascontiguousarray(words, np.int32)
    state = dict(head=w[:, 0].copy(), valid=w[:, 1].copy(), prev=w.view(F64)[:, 1:].copy())
    return N.nav_step(setup.route, setup.cmd, setup.length, pose, state, xy_scale=setup.xy_scale, **setup.nav)


def nav_words(state):
    w = np.zeros((len(state["head"]), 8), np.int32)
    w[:, 0], w[:, 1] = state["head"], state["valid"]
    w.view(F64)[:, 1:] = state["prev"]
    return w


def _rows(cands):
    c = np.asarray(cands, F32)
    return c.reshape(-1, c.shape[-2], c.shape[-1])


def select_stage(setup, cands, target, discs, slots):
    """Selection cost v2 against the guide's discs and capsules: select_guide_ref.select with capsule_ref's term in the violation,
    the bound of select_guide_ref.cost_bound with capsule_ref.cost_bound as the violation's, and per scene `clear`: every hinge
    further from its kink than twice its fp32 error (select_guide_ref.hinges_clear; capsule_ref.hinge_margin against phi_bound)
    and the two smallest costs of the searched set more than select_guide_ref.GAP bounds apart."""
    S, K = setup.S, setup.K
    t = _rows(cands)
    H = t.shape[1]
    c = None if slots is None else CR.capsules(slots)
    w, hard = setup.weights, setup.hard
    with np.errstate(all="ignore"), CR._capsuled(c):
        res = SG.select(t, S, target, w, hard, discs, None)
    wg, ws, wc, wv = (abs(float(F32(v))) for v in w)
    b1 = SR.cost_bound(K, H, w[:3], target is not None)
    if wv == 0.0:
        bound = np.full((S, K), b1)
    else:                                                # select_guide_ref.cost_bound, line by line, with the capsules' share
        t1 = 8.0 * (wg if target is not None else 0.0) + 32.0 * (ws if H >= 3 else 0.0) + 8.0 * wc
        with np.errstate(all="ignore"):
            bv = CR.cost_bound(t, discs, None, None, None, c, None).reshape(K, S).T
        v = res["violation"]
        ep = wv * bv + SG.U * wv * (v + bv)
        bound = b1 + ep + SG.U * (t1 + b1 + wv * v + ep)
    t4 = t.reshape(K, S, H, -1)
    clear = np.ones(S, bool)
    for s in range(S):
        if discs is not None:
            clear[s] &= SG.hinges_clear(t4[:, s], np.asarray(discs, F32)[s:s + 1], None)
        if c is not None:
            one = dict(slots=c["slots"][s:s + 1], weight=c["weight"])
            x, y = t4[:, s, :, 0].astype(F64), t4[:, s, :, 1].astype(F64)
            with np.errstate(all="ignore"):
                margin = CR.hinge_margin(one, x, y)                                  # inf where a slot is empty: no kink there
                clear[s] &= bool((margin > 2.0 * np.where(np.isfinite(margin), CR.phi_bound(one, x, y), 0.0)).all())
        cost = res["cost"][s]
        searched = np.sort(cost[SG.searched(res["cost"], res["free"], hard)[s]])
        if searched.size > 1:
            clear[s] &= bool(searched[1] - searched[0] > SG.GAP * bound[s].max())
    res.update(bound=bound, clear=clear)
    return res


def commit_stage(setup, cands, cost, selected, active, words, motion):
    """commit_ref.commit in fp64 on the device's fp32 cost, index and active; `bound` = dist2_bound at the tick's own odometry,
    `unclear` [S] = commit_ref.unclear."""
    c = setup.commit
    t = _rows(cands)
    H = t.shape[1]
    with np.errstate(all="ignore"):
        res = CM.commit(t, setup.S, cost, selected, words, active=active, motion=motion, h0=c["h0"], shift=c["shift"],
                        max_hold=c["max_hold"], radius=c["radius"], margin=c["margin"], ratio=c["ratio"], dtype=F64)
    t_max = 1.0 if motion is None else float(np.abs(np.asarray(motion, F64)[:, :2]).max())
    res["bound"] = CM.dist2_bound(H, c["h0"], c["shift"], t_max)
    res["unclear"] = CM.unclear(res, res["bound"], c["radius"])
    return res


def modes_stage(setup, cands):
    """modes_ref.modes; `clear` [S]: every pair's distance further from r2 than twice modes_ref.bound (tests/test_gpu_modes.py)."""
    m = setup.modes
    t = _rows(cands)
    with np.errstate(all="ignore"):
        res = MO.modes(t, setup.S, m["M"], m["radius"], m["h0"])
        res["clear"] = MO.margins(t, setup.S, m["radius"], m["h0"]) > 2.0 * MO.bound(t.shape[1], m["h0"])
    return res


def stop_stage(setup, plan, discs, slots):
    """fallback_ref.stop_short in float32: the kernel's bits (tests/test_gpu_fallback.py compares bit for bit)."""
    c = None if slots is None else CR.capsules(slots)
    return FB.stop_short(np.asarray(plan, F32), FB.guide(discs=discs, capsules=c), setup.stop_params, F32)


def _angle_error(b):
    """control_ref's e_angle, and for a vector that is exactly zero on both sides (two waypoints that are the same fp32 numbers,
    as a plan re-timed to a halt has them: the same products and an exact difference) atan2(0, 0) = 0 on both: what is left is
    the 16 u of the angle's own arithmetic."""
    inner = b.e_angle
    return lambda e_v, r: 16.0 * CT.U if r == 0.0 else inner(e_v, r)


def control_stage(setup, turn, speed_w, plan, velocity, target):
    """control_ref.tick per scene from the recorded windows.  dict(control [S, 3] fp64, turn, speed_w: the new windows, steer,
    throttle, e_a, e_delta: the bounds [S], clear_steer and clear_brake [S]: the margins of the decisions the steer (aim,
    to_target) and the pedals (brake) hang on above twice their allowance (tests/test_control_device_cpu.py), info)."""
    p, S = setup.control, setup.S
    out = dict(control=np.zeros((S, 3)), turn=np.zeros(np.shape(turn), F64), speed_w=np.zeros(np.shape(speed_w), F64), steer=np.zeros(S),
               throttle=np.zeros(S), e_a=np.zeros(S), e_delta=np.zeros(S), clear_steer=np.ones(S, bool), clear_brake=np.ones(S, bool),
               info=[])
    for s in range(S):
        st = SimpleNamespace(turn=np.asarray(turn[s], F64).copy(), speed=np.asarray(speed_w[s], F64).copy())
        v = float(F32(velocity[s]))
        u, info = CT.tick(p, st, np.asarray(plan[s], F32), v, None if target is None else np.asarray(target[s], F32))
        norms = [n for n in info.norms if n > 0.0]
        b = CT.bound(p, info.scale, abs(v), min(norms) if norms else 1.0, target is not None)
        b.e_angle = _angle_error(b)
        with np.errstate(all="ignore"):
            ms = CT.margins(p, info, b, target is not None)
        sound = bool(np.isfinite(b.steer) and b.e_a > 0 and np.isfinite(b.throttle))      # a vector shorter than its own error: no bound
        out["clear_steer"][s] = sound and all(ms[k][0] > 2.0 * ms[k][1] for k in ("aim", "to_target"))
        out["clear_brake"][s] = sound and ms["brake"][0] > 2.0 * ms["brake"][1]
        out["control"][s], out["turn"][s], out["speed_w"][s] = u, st.turn, st.speed
        out["steer"][s], out["throttle"][s], out["e_a"][s], out["e_delta"][s] = b.steer, b.throttle, b.e_a, b.e_delta
        out["info"].append(info)
    return out


def vehicle_stage(setup, words, control, hold):
    return V.step(V.unpack_state(words), np.asarray(control, F32), hold, **setup.vehicle)


def world_stage(world, dt):
    """`World.advance`: every centre moved by dt times its velocity.  (out, bound): a product and a sum, or one fused operation:
    one rounding of the product apart, and the sum's own."""
    if world is None:
        return None, None
    w = np.asarray(world, F64)
    out = w.copy()
    step = float(dt) * w[..., 2:4]
    out[..., 0:2] = w[..., 0:2] + step
    bound = np.zeros(w.shape)
    with np.errstate(invalid="ignore"):
        bound[..., 0:2] = np.nan_to_num(np.spacing(np.abs(out[..., 0:2])) + E52 * np.abs(step), nan=0.0, posinf=0.0)
    return out, bound


def metrics_stage(setup, words, pose, velocity, yaw_rate, discs, boxes):
    """drive_ref.step per scene from the recorded record words: (records, clear [S]: drive_ref.Clear's value per scene)."""
    recs, clear = DR.unpack(words), np.zeros(setup.S)
    out = []
    for s in range(setup.S):
        c = DR.Clear()
        out.append(DR.step(recs[s], setup.metrics, pose[s], velocity[s], yaw_rate[s], setup.route[s], setup.length[s], setup.cum[s],
                           None if discs is None else discs[s], None if boxes is None else boxes[s], c))
        clear[s] = c.value
    return out, clear


def metrics_scale(setup):
    """R of drive_ref.accumulator_bound, as tests/test_gpu_drive.py forms it for its random drives: the route's extent and the
    largest quotient of a speed by dt twice."""
    r, dt = setup.route, setup.metrics["dt"]
    return float(max(np.ptp(r[..., 0]) + np.ptp(r[..., 1]) + 8.0, 4.0 * setup.vehicle.get("v_max", V.DEFAULTS["v_max"]) / dt / dt))


# ---- a drive on the CPU ------------------------------------------------------------------------------------------------------------
def roll(setup, pose, world_discs, world_boxes, source, ticks):
    """`simulation.drive` with the restatements in the kernels' places: `source(t, pose, nav) -> candidates [K, S, H, D]` float32
    in model units stands in for the sampler.  Returns the transcript.  What a kernel keeps in float32 is rounded to float32."""
    S = setup.S
    veh = V.pack_state(V.reset(V.fresh_state(S), pose))
    pose, velocity = np.asarray(pose, F64).copy(), np.zeros(S, F32)
    navw, comw = np.zeros((S, 8), np.int32), CM.fresh_state(S, setup.H)
    turn, speed_w = np.zeros((S, setup.control.n_turn), F32), np.zeros((S, setup.control.n_speed), F32)
    met, done = DR.pack([DR.fresh() for _ in range(S)]), np.zeros(S, np.int32)
    wd = None if world_discs is None else np.asarray(world_discs, F64).copy()
    wb = None if world_boxes is None else np.asarray(world_boxes, F64).copy()
    recs = []
    for t in range(ticks):
        r = dict(pose=pose, velocity=velocity, world_discs=wd, world_boxes=wb, nav_words=navw, commit_words=comw, turn=turn,
                 speed_w=speed_w, veh_words=veh, met_words=met, done_prev=done)
        g = guide_stage(pose, wd, wb, setup.xy_scale, setup.waypoint_dt)
        r["g_discs"], r["g_slots"] = g["discs"], g["slots"]
        nav = nav_stage(setup, pose, navw)
        navw = nav_words(nav["state"])
        r.update(nav_words_after=navw, target=nav["target"], window=nav["window"], motion=nav["motion"])
        cands = np.ascontiguousarray(source(t, pose, nav), F32)
        sel = select_stage(setup, cands, nav["target"], g["discs"], g["slots"])
        cost = sel["cost"].astype(F32)
        r.update(cands=cands, cost=cost, active=sel["active"].astype(np.int32), selected=sel["index"])
        com = commit_stage(setup, cands, cost, sel["index"], r["active"], comw, nav["motion"])
        comw = com["state"]
        r.update(c_index=com["index"], c_status=com["status"], c_follower=com["follower"], c_dist2=com["dist2"].astype(F32),
                 c_blocked=com["blocked"], index=com["index"], blocked=com["blocked"], commit_words_after=comw)
        mo = modes_stage(setup, cands)
        r.update(m_modes=mo["modes"].reshape(-1, S, setup.H, setup.D), m_index=mo["index"], m_mass=mo["mass"], m_assign=mo["assign"],
                 m_count=mo["count"])
        st = stop_stage(setup, com["best"], g["discs"], g["slots"])
        r.update(traj=st["out"], f_first=st["first"], f_status=st["status"], f_stop_at=st["stop_at"], f_after=st["active_after"])
        ctl = control_stage(setup, turn, speed_w, st["out"], velocity, nav["target"])
        turn, speed_w = ctl["turn"].astype(F32), ctl["speed_w"].astype(F32)
        r.update(control=ctl["control"].astype(F32), turn_after=turn, speed_w_after=speed_w)
        v = vehicle_stage(setup, veh, r["control"], done)
        veh, pose, velocity = V.pack_state(v["state"]), v["pose"], v["velocity"]
        wd, wb = world_stage(wd, setup.vehicle["dt"])[0], world_stage(wb, setup.vehicle["dt"])[0]
        new, _ = metrics_stage(setup, met, pose, velocity, v["yaw_rate"], wd, wb)
        met = DR.pack(new)
        done = met[:, 2].copy()
        r.update(veh_words_after=veh, pose_after=pose, velocity_after=velocity, yaw_after=v["yaw_rate"], met_words_after=met, done=done,
                 world_discs_after=wd, world_boxes_after=wb)
        recs.append(r)
    return dict(setup=setup, ticks=recs)


# ---- the replay --------------------------------------------------------------------------------------------------------------------
DEFAULT = {
    "guide.pose": "pose",                # the pose before the vehicle step
    "guide.world": "world",              # the world before `advance`
    "guide.dt": "waypoint_dt",           # what scales obstacle velocities
    "nav.pose": "pose",
    "stop.plan": "committed",            # the commit's plan
    "control.plan": "traj",              # the returned trajectory, which is the fallback's output
    "vehicle.control": "control",        # this tick's last_control
    "vehicle.hold": "done_prev",         # the previous tick's done
    "metrics.world": "world_next",       # the advanced world
}
DEFECTS = {
    "a: navigator stepped on the pose after the vehicle moved": {"nav.pose": "pose_next"},
    "b: guide built from the advanced world": {"guide.world": "world_next"},
    "c: controller fed candidate 0": {"control.plan": "candidate0"},
    "d: controller fed the plan from before the fallback": {"control.plan": "committed"},
    "e: vehicle fed the previous tick's control": {"vehicle.control": "control_prev"},
    "f: vehicle held by this tick's done": {"vehicle.hold": "done"},
    "g: metrics fed the world before it advanced": {"metrics.world": "world"},
    "h: obstacle velocities scaled by the vehicle's dt": {"guide.dt": "vehicle_dt"},
}


def _bits(a):
    a = np.ascontiguousarray(a)
    if a.dtype.kind == "f":
        return a.view(np.int32 if a.dtype.itemsize == 4 else np.int64)
    return a.astype(np.int64) if a.dtype.kind in "iub" else a


class Report:
    """What a replay found: `failures` (tick, stage, what, detail), `worst` error-to-bound ratio per stage, `decisions`, the
    droppable decision comparisons met, and `dropped` (tick, stage, scene) of those left out for want of clearance."""

    def __init__(self):
        self.failures, self.worst, self.decisions, self.dropped = [], {}, 0, []
        self.exact = 0

    def fail(self, t, stage, what, detail=None):
        self.failures.append((t, stage, what, detail))

    def same(self, t, stage, what, got, want):
        """Bit for bit."""
        self.exact += 1
        g, w = _bits(got), _bits(want)
        if g.shape != w.shape or not np.array_equal(g, w):
            self.fail(t, stage, what, (np.asarray(got).tolist(), np.asarray(want).tolist()) if np.size(got) <= 16 else None)

    def within(self, t, stage, what, got, want, bound):
        got, want, bound = np.asarray(got, F64), np.asarray(want, F64), np.asarray(bound, F64)
        if got.shape != want.shape:
            return self.fail(t, stage, what, ("shape", got.shape, want.shape))
        both = (np.isnan(got) & np.isnan(want)) | (got == want)
        with np.errstate(invalid="ignore"):
            err = np.where(both, 0.0, np.abs(got - want))
            ratio = np.where(err == 0.0, 0.0, err / np.maximum(bound, 1e-300))
        worst = float(np.max(ratio)) if ratio.size else 0.0
        self.worst[stage] = max(self.worst.get(stage, 0.0), worst if np.isfinite(worst) else np.inf)
        if not (err <= bound).all():
            self.fail(t, stage, what, worst)

    def decide(self, t, stage, s, clear):
        """Counts one droppable decision comparison; False where it is dropped."""
        self.decisions += 1
        if not clear:
            self.dropped.append((t, stage, s))
        return bool(clear)

    @property
    def ok(self):
        return not self.failures

    def summary(self):
        frac = len(self.dropped) / max(self.decisions, 1)
        return (f"{len(self.failures)} failures; dropped {len(self.dropped)} of {self.decisions} decision comparisons ({100 * frac:.1f} %); "
                f"worst error / bound per stage: " + ", ".join(f"{k} {v:.3g}" for k, v in sorted(self.worst.items())))


def _committed(r, S):
    return np.stack([r["cands"][int(r["c_index"][s]), s] for s in range(S)])


def _source(name, r, prev, setup):
    S = setup.S
    if name == "pose":
        return r["pose"]
    if name == "pose_next":
        return r["pose_after"]
    if name == "world":
        return r["world_discs"], r["world_boxes"]
    if name == "world_next":
        return r["world_discs_after"], r["world_boxes_after"]
    if name == "waypoint_dt":
        return setup.waypoint_dt
    if name == "vehicle_dt":
        return setup.vehicle["dt"]
    if name == "traj":
        return r["traj"]
    if name == "committed":
        return _committed(r, S)
    if name == "candidate0":
        return r["cands"][0]
    if name == "control":
        return r["control"]
    if name == "control_prev":
        return np.zeros((S, 3), F32) if prev is None else prev["control"]
    if name == "done_prev":
        return r["done_prev"]
    if name == "done":
        return r["done"]
    raise KeyError(name)


CARRIED = (("pose", "pose_after"), ("velocity", "velocity_after"), ("world_discs", "world_discs_after"), ("world_boxes", "world_boxes_after"),
           ("nav_words", "nav_words_after"), ("commit_words", "commit_words_after"), ("turn", "turn_after"), ("speed_w", "speed_w_after"),
           ("veh_words", "veh_words_after"), ("met_words", "met_words_after"), ("done_prev", "done"))


def replay(transcript, wiring=DEFAULT):
    """Every stage of every tick on its recorded inputs, as `wiring` routes them, against its recorded outputs.  Returns a Report."""
    setup, ticks = transcript["setup"], transcript["ticks"]
    wiring = dict(DEFAULT, **wiring)
    S, K, H = setup.S, setup.K, setup.H
    rep = Report()
    R = metrics_scale(setup)
    prev = None
    for t, r in enumerate(ticks):
        src = lambda key: _source(wiring[key], r, prev, setup)  # noqa: E731
        # -- what a tick starts from is what the tick before left: nothing in between moved a state
        if prev is not None:
            for a, b in CARRIED:
                if r.get(a) is not None or prev.get(b) is not None:
                    rep.same(t, "carry", a, r[a], prev[b])
        # -- guide
        wd, wb = src("guide.world")
        g = guide_stage(src("guide.pose"), wd, wb, setup.xy_scale, src("guide.dt"))
        if g["discs"] is not None or r.get("g_discs") is not None:
            rep.within(t, "guide", "discs", r["g_discs"], g["discs"], g["discs_bound"])
        if g["slots"] is not None or r.get("g_slots") is not None:
            live = (g["boxes"][..., 6] > 0) & (g["boxes"][..., 7] > 0)
            rep.same(t, "guide", "an empty box is seven zeros", r["g_slots"][~live], g["slots"][~live])
            rep.same(t, "guide", "radii", r["g_slots"][..., 6], g["slots"][..., 6])
            rep.within(t, "guide", "slots", np.where(live[..., None], r["g_slots"], 0), np.where(live[..., None], g["slots"], 0),
                       slots_bound(g, r["g_slots"]))
        # -- navigator: the walk's integers and the state exactly (tests/test_gpu_nav.py), the fp32 outputs within their bounds
        nav = nav_stage(setup, src("nav.pose"), r["nav_words"])
        after = np.ascontiguousarray(r["nav_words_after"], np.int32)
        rep.same(t, "nav", "head", after[:, 0], nav["state"]["head"])
        rep.same(t, "nav", "valid", after[:, 1], nav["state"]["valid"])
        rep.same(t, "nav", "the pose it stepped on", after.view(F64)[:, 1:], nav["state"]["prev"])
        for name in ("target", "window", "motion"):
            rep.within(t, "nav", name, r[name], nav[name], nav[name + "_bound"])
        # -- pin: a pinned cell of every candidate holds the known value (|known| <= 1, outside [0, :3])
        if r.get("pin_known") is not None:
            known, mask = r["pin_known"], r["pin_mask"] == 1.0
            mask = mask & (np.abs(known) <= 1.0)
            mask[:, 0, :3] = False
            rep.same(t, "pin", "pinned cells", np.where(mask[None], r["cands"], 0), np.broadcast_to(np.where(mask, known, 0)[None], r["cands"].shape))
        # -- selection
        sel = select_stage(setup, r["cands"], r["target"], r["g_discs"], r["g_slots"])
        finite = np.isfinite(sel["cost"])
        rep.within(t, "select", "cost", np.where(finite, r["cost"], 0), np.where(finite, sel["cost"], 0), sel["bound"])
        rep.same(t, "select", "finite costs", np.isfinite(r["cost"]), finite)
        for s in range(S):
            if rep.decide(t, "select", s, sel["clear"][s]):
                rep.same(t, "select", f"active, scene {s}", r["active"][s], sel["active"][s])
                rep.same(t, "select", f"index, scene {s}", r["selected"][s], sel["index"][s])
        # -- commit, on the device's own cost, index and active
        com = commit_stage(setup, r["cands"], r["cost"], r["selected"], r["active"], r["commit_words"], r["motion"])
        ok = com["finite"] & com["prior_ok"][:, None]
        rep.within(t, "commit", "dist2", np.where(ok, r["c_dist2"], 0), np.where(ok, com["dist2"], 0), com["bound"])
        for s in range(S):
            if rep.decide(t, "commit", s, not com["unclear"][s]):
                for name, key in (("index", "c_index"), ("status", "c_status"), ("follower", "c_follower"), ("blocked", "c_blocked")):
                    rep.same(t, "commit", f"{name}, scene {s}", r[key][s], com[name][s])
                rep.same(t, "commit", f"state, scene {s}", r["commit_words_after"][s], com["state"][s])
        rep.same(t, "commit", "Selection.index is the committed one", r["index"], r["c_index"])
        rep.same(t, "commit", "Selection.blocked is the committed one", r["blocked"], r["c_blocked"])
        # -- modes
        mo = modes_stage(setup, r["cands"])
        for s in range(S):
            if rep.decide(t, "modes", s, mo["clear"][s]):
                for name in ("index", "mass", "assign", "count"):
                    rep.same(t, "modes", f"{name}, scene {s}", r["m_" + name][s], mo[name][s])
                rep.same(t, "modes", f"rows, scene {s}", r["m_modes"][:, s], mo["modes"].reshape(-1, S, H, setup.D)[:, s])
        # -- stop-short: bit for bit, and what the call returned is its output
        st = stop_stage(setup, src("stop.plan"), r["g_discs"], r["g_slots"])
        rep.same(t, "stop", "the returned trajectory", r["traj"], st["out"])
        for name, key in (("first", "f_first"), ("status", "f_status"), ("stop_at", "f_stop_at"), ("active_after", "f_after")):
            rep.same(t, "stop", name, r[key], st[name])
        # -- controller
        ctl = control_stage(setup, r["turn"], r["speed_w"], src("control.plan"), r["velocity"], r["target"])
        got = np.asarray(r["control"], F64)
        for s in range(S):
            rep.decide(t, "control", s, ctl["clear_steer"][s] and ctl["clear_brake"][s])
            if ctl["clear_steer"][s]:
                rep.within(t, "control", f"steer, scene {s}", got[s, 1], ctl["control"][s, 1], ctl["steer"][s])
                rep.within(t, "control", f"turn window: the new sample, scene {s}", r["turn_after"][s, -1], ctl["turn"][s, -1], ctl["e_a"][s])
            if ctl["clear_brake"][s]:
                rep.same(t, "control", f"brake, scene {s}", got[s, 2], ctl["control"][s, 2])
                rep.within(t, "control", f"throttle, scene {s}", got[s, 0], ctl["control"][s, 0], ctl["throttle"][s])
        rep.within(t, "control", "speed window: the new sample", r["speed_w_after"][:, -1], ctl["speed_w"][:, -1], ctl["e_delta"])
        for key in ("turn", "speed_w"):
            rep.same(t, "control", f"{key}: the older samples", r[key + "_after"][:, :-1], r[key][:, 1:])
        # -- vehicle: the speed and everything a hold writes exactly, the pose within its bound (tests/test_gpu_vehicle.py)
        v = vehicle_stage(setup, r["veh_words"], src("vehicle.control"), src("vehicle.hold"))
        got = V.unpack_state(r["veh_words_after"])
        rep.same(t, "vehicle", "speed", got["speed"], v["state"]["speed"])
        rep.same(t, "vehicle", "valid", got["valid"], v["state"]["valid"])
        rep.same(t, "vehicle", "velocity", r["velocity_after"], v["velocity"])
        rep.within(t, "vehicle", "pose", r["pose_after"], v["pose"], v["pose_bound"])
        rep.within(t, "vehicle", "yaw rate", r["yaw_after"], v["yaw_rate"], v["yaw_bound"])
        rep.same(t, "vehicle", "the state is the pose written out", np.stack([got["x"], got["y"], got["compass"]], axis=1), r["pose_after"])
        # -- world
        for name in ("world_discs", "world_boxes"):
            if r.get(name) is not None:
                out, bound = world_stage(r[name], setup.vehicle["dt"])
                rep.within(t, "world", name, r[name + "_after"][..., :2], out[..., :2], bound[..., :2])
                rep.same(t, "world", name + ": all but the centres", r[name + "_after"][..., 2:], r[name][..., 2:])
        # -- metrics: every integer word exactly, the fp64 words within the accumulators' bound (tests/test_gpu_drive.py)
        wd, wb = src("metrics.world")
        recs, clear = metrics_stage(setup, r["met_words"], r["pose_after"], r["velocity_after"], r["yaw_after"], wd, wb)
        want, gotw = DR.pack(recs), np.ascontiguousarray(r["met_words_after"], np.int32)
        gr = DR.unpack(gotw)
        for s in range(S):
            if rep.decide(t, "metrics", s, clear[s] > METRICS_CLEAR):
                rep.same(t, "metrics", f"integer words, scene {s}", gotw[s, :10], want[s, :10])
                rep.same(t, "metrics", f"done, scene {s}", r["done"][s], want[s, 2])
                T = max(int(want[s, 1]), 1)
                for k in DR.SUMS + DR.SQUARES:
                    b = DR.squares_bound(T, R) if k in DR.SQUARES else DR.accumulator_bound(T, R)
                    rep.within(t, "metrics", f"{k}, scene {s}", gr[s][k], recs[s][k], b)
        prev = r
    return rep


# ---- what a transcript must contain for a replay of it to mean something -----------------------------------------------------------
def preconditions(transcript):
    """The observed values the tests assert on: dict(retimed, held_or_changed, nonzero_selected, control_changes, ended, moved)."""
    ticks, S = transcript["ticks"], transcript["setup"].S
    retimed = sum(int((r["f_status"] != 0).sum()) for r in ticks)
    differ = sum(int((r["c_index"] != r["selected"]).sum()) for r in ticks)
    changed = sum(int(not np.array_equal(r["commit_words"], r["commit_words_after"])) for r in ticks)
    nonzero = sum(int((r["selected"] != 0).sum()) for r in ticks)
    moves = sum(int((_bits(a["control"]) != _bits(b["control"])).any()) for a, b in zip(ticks, ticks[1:]))
    ended = [next((t for t, r in enumerate(ticks) if r["done"][s] != 0), None) for s in range(S)]
    moved = any(r.get(k) is not None and not np.array_equal(r[k], r[k + "_after"]) for r in ticks for k in ("world_discs", "world_boxes"))
    statuses = sorted({int(v) for r in ticks for v in r["c_status"]})
    return dict(retimed=retimed, committed_differs=differ, commit_state_changed=changed, nonzero_selected=nonzero, control_changes=moves,
                of=len(ticks) - 1, ended=ended, done=[int(v) for v in ticks[-1]["done"]], obstacles_moved=bool(moved),
                commit_statuses=statuses)


# ---- the scenario the CPU and the GPU test share -----------------------------------------------------------------------------------
XY_SCALE = 23.315
S, K, H, D, TICKS, DT = 3, 4, 16, 7, 10, 0.25
G_POINTS = 60
R_EGO = 2.0


def routes():
    """Three gently curving routes of 60 points 2 m apart and start poses on their first point heading along them: the forward
    vector (sin c, -cos c) is the first segment's direction at c = atan2(dx, -dy)."""
    k = np.arange(G_POINTS)
    heading = np.stack([0.3 + 0.004 * k, -1.0 - 0.006 * k, 2.2 + 0.005 * k])
    step = 2.0 * np.stack([np.cos(heading), np.sin(heading)], axis=-1)
    route = np.array([[10.0, -5.0], [-40.0, 25.0], [30.0, 60.0]])[:, None] + np.cumsum(step, axis=1) - step[:, :1]
    d = route[:, 1] - route[:, 0]
    pose = np.concatenate([route[:, 0], np.arctan2(d[:, 0], -d[:, 1])[:, None]], axis=1)
    return route, pose


def world(route):
    """discs [3, 2, 5] and boxes [3, 2, 7] in world metres.  Scene 0: a disc of radius 4.5 standing on the route 18 m ahead, over
    the route points from 14 to 22 m (a plan pinned onto the route points beyond the navigator's 7 m meets it as soon as the
    ego has moved 1 m); a slow box far off to the side.  Scene 1: a disc of radius 0.4 that crosses the route
    line 1 m BEHIND the start at 20 m/s, from 15 m to the left: it is on the line after three ticks of 0.25 s and within reach
    (0.4 + r_ego = 2.4 m) at that tick alone, when an ego that started from rest has moved less than 1.4 m; a plan's waypoints lie
    ahead of the ego, so a plan drawn along the route is not stopped by it and the ego is under way at the contact.  Scene 2: a disc that crosses well behind the ego and a box that drives
    beside the route, 9 m off it: nothing in the way.  Every scene's second disc slot and the unused box slots are empty."""
    discs, boxes = np.zeros((S, 2, 5)), np.zeros((S, 2, 7))
    discs[:, :, 4] = -1.0
    unit = lambda s, i: (route[s, i + 1] - route[s, i]) / np.linalg.norm(route[s, i + 1] - route[s, i])  # noqa: E731
    left = lambda u: np.array([-u[1], u[0]])  # noqa: E731
    discs[0, 0] = [*route[0, 9], 0.0, 0.0, 4.5]
    discs[1, 0] = [*(route[1, 0] - 1.0 * unit(1, 0) + 15.0 * left(unit(1, 0))), *(-20.0 * left(unit(1, 0))), 0.4]
    discs[2, 0] = [*(route[2, 0] - 14.0 * unit(2, 0) + 6.0 * left(unit(2, 0))), *(-1.5 * left(unit(2, 0))), 1.0]
    u0, u2 = unit(0, 0), unit(2, 0)
    boxes[0, 0] = [*(route[0, 2] + 15.0 * left(u0)), *(0.5 * u0), np.arctan2(u0[1], u0[0]), 4.5, 2.0]
    boxes[2, 1] = [*(route[2, 1] + 9.0 * left(u2)), *(3.0 * u2), np.arctan2(u2[1], u2[0]), 4.5, 2.0]
    return discs, boxes


def setup(control_cfg, waypoint_dt=None):
    """The Setup of the scenario; `control_cfg` is a config with PID and CONTROL (the package's create_cfg())."""
    route, _ = routes()
    gap_m, decel = 1.5, 4.0
    wdt = DT if waypoint_dt is None else float(waypoint_dt)
    stop = np.array([[gap_m / XY_SCALE, decel * wdt * wdt / XY_SCALE]] * S, F64).astype(F32)
    return Setup(S=S, K=K, H=H, D=D, xy_scale=XY_SCALE, waypoint_dt=wdt, route=route, cmd=np.zeros((S, G_POINTS), np.int32),
                 length=np.full(S, G_POINTS, np.int32), nav=dict(min_distance=7.0, max_distance=50.0, R=16, first=0),
                 weights=(1.0, 0.5, 0.25, 2.0), hard=True,
                 # the procedural weights' candidates lie about 1.4 model units (rms) from the plan of the tick before: a radius that some meet
                 commit=dict(radius=1.5, margin=0.01, ratio=0.2, max_hold=0, h0=1, shift=1),
                 modes=dict(M=3, radius=2.0 / XY_SCALE, h0=1), stop_params=stop,
                 control=CT.params(control_cfg, waypoints=4, post="agent", source="pid", sign_x=-1.0, target_scale=1.0, xy_scale=XY_SCALE),
                 vehicle=dict(V.DEFAULTS, dt=DT),
                 metrics=dict(DR.CFG, dt=DT, stop_on_collision=True, r_ego=R_EGO))
