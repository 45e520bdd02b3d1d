"""CPU: the restatement of "signals v1" (tests/signals_ref.py) against records derived by hand -- a timed light that is run, a
stop sign that is run and one that is obeyed, stop_on_yellow, overflow, hold, a negative offset, every kind of empty slot --, the
conditions the GPU comparison needs of the random drives, and every refusal of `Signals`, `World` and the C entry points, which are
all raised before a launch.

The common setup: the ego at compass pi/2, so forward is +x; x_k = 0.125 + 1.5 k, y = 0, dt = 0.5, probe = -2 (the probe is at
x_k - 2), margin = 3."""
import ctypes as C

import numpy as np
import pytest
import torch

import signals_ref as R


@pytest.fixture(scope="module")
def built():
    import __graft_entry__ as g
    g.build()
    from autonomous_driving_with_diffusion_model_amd import _lib
    return _lib


def _ints(state):
    return {k: int(state[k][0]) for k in R.INTS}


def _emitting(outs):
    return [t for t, o in enumerate(outs) if o["emit"].any()]


ZERO = {k: 0 for k in R.INTS}


def test_scenario_a_a_timed_light_is_run_once_and_only_the_light_that_governs_binds():
    """Slot 0 at x = 12 is green for 2 s, yellow for 1 s, red for 5 s: red from step 6 (t = 3 s) on.  The ego passes the line
    between steps 7 (x = 10.625) and 8 (x = 12.125), so the line binds at steps 6 and 7 only; the probe (x_k - 2) passes it between
    steps 9 (11.625) and 10 (13.125), at t = 5 s: red.  The always green light at x = 24 is crossed at step 18 without a run; the
    red one in the other lane (lat = 10 > L = 4) and the red one facing the other way (head = -1, and crossed from the wrong side)
    never bind and are never run."""
    rec, (poses, vel) = R.scenario_a()
    outs = R.run(rec, poses, vel, **R.CFG)
    assert _ints(outs[-1]["state"]) == dict(ZERO, ticks=23, have=1, red_runs=1, first_tick=10, first_slot=0)
    assert outs[10]["phase"].tolist() == [[3, 1, 3, 3]] and outs[10]["red"].tolist() == [1]
    assert _emitting(outs) == [6, 7] and all(outs[t]["emit"].tolist() == [[True, False, False, False]] for t in (6, 7))
    assert [o["phase"][0, 0] for o in outs[:8]] == [1, 1, 1, 1, 2, 2, 3, 3]
    assert [int(o["state"]["emitted"][0]) for o in outs] == [0] * 6 + [1, 1] + [0] * 16
    assert outs[-1]["state"]["qx"][0] == 0.125 + 1.5 * 23 - 2.0 and abs(outs[-1]["state"]["qy"][0]) < 1e-15
    # the plane of step 6: 3 m short of the line, 9 - 9.125 m ahead of the ego, whose forward axis is ego +y
    pl = outs[6]["planes"][0]
    assert abs(pl[0, 0]) < 1e-7 and pl[0, 1] == 1.0 and pl[0, 2] == np.float32((9.0 - 9.125) / R.CFG["xy_scale"])
    assert (pl[1:] == np.array(R.INERT, dtype=np.float32)).all() and (outs[5]["planes"] == np.array(R.INERT, dtype=np.float32)).all()


def test_scenario_a_with_stop_on_yellow_binds_from_the_yellow_on():
    rec, (poses, vel) = R.scenario_a()
    outs = R.run(rec, poses, vel, **dict(R.CFG, stop_on_yellow=True))
    assert _emitting(outs) == [4, 5, 6, 7] and _ints(outs[-1]["state"])["red_runs"] == 1


def test_scenario_b_a_stop_sign_is_run_at_constant_speed_and_obeyed_with_a_stop():
    """The sign at x = 12 with reach 10 gates x in [2, 12]: steps 2 .. 7.  Step 2 takes it as the target; at step 8 (x = 12.125)
    the ego is beyond the line: a run without a stop, none with the velocity 0.0 reported at step 5 -- from which step on the
    sign no longer emits."""
    rec, (poses, vel) = R.scenario_b()
    outs = R.run(rec, poses, vel, **R.CFG)
    assert _ints(outs[-1]["state"]) == dict(ZERO, ticks=11, have=1, stop_runs=1, stops_met=1, first_tick=8, first_slot=0)
    assert _emitting(outs) == [2, 3, 4, 5, 6, 7] and [int(o["state"]["target"][0]) for o in outs] == [0, 0] + [1] * 6 + [0] * 4
    assert (outs[3]["phase"] == 4).all() and outs[8]["ran"].tolist() == [1]
    rec, (poses, vel) = R.scenario_b(stop_at=5)
    outs = R.run(rec, poses, vel, **R.CFG)
    assert _ints(outs[-1]["state"]) == dict(ZERO, ticks=11, have=1, stops_met=1, stop_done=1)
    assert _emitting(outs) == [2, 3, 4] and outs[8]["completed"].tolist() == [1]
    # a velocity that is not a number is not below the threshold
    vel[5] = np.nan
    assert _ints(R.run(rec, poses, vel, **R.CFG)[-1]["state"])["stop_runs"] == 1
    # a target left sideways is cleared without a run: the ego changes lanes at step 6 (lat = 2 - 5 < 0)
    rec, (poses, vel) = R.scenario_b()
    poses[6:, 0, 1] = 5.0
    outs = R.run(rec, poses, vel, **R.CFG)
    assert _ints(outs[-1]["state"]) == dict(ZERO, ticks=11, have=1, stops_met=1) and _emitting(outs) == [2, 3, 4, 5]


def test_more_binding_lines_than_planes_keep_the_lowest_and_set_the_flag_for_good():
    rec = np.zeros((1, 3, 10))
    rec[0, 0] = R.from_lines([14.0, 0.0], 0.0, 4.0, R.LIGHT, 20.0, [0.0, 0.0, 0.0, 1.0])
    rec[0, 1] = R.from_lines([40.0, 0.0], 0.0, 4.0, R.LIGHT, 20.0, [0.0, 0.0, 0.0, 1.0])      # out of reach
    rec[0, 2] = R.from_lines([12.0, 0.0], 0.0, 4.0, R.LIGHT, 20.0, [0.0, 0.0, 0.0, 1.0])
    poses, vel = R.straight_drive(12)
    outs = R.run(rec, poses, vel, **dict(R.CFG, planes=1))
    assert [o["overflow"][0] for o in outs] == [1] * 8 + [0] * 4 and all(o["state"]["flags"][0] == 1 for o in outs)
    assert [int(o["state"]["emitted"][0]) for o in outs] == [1] * 10 + [0, 0]       # slot 0 until x > 14 (step 10), then nothing
    assert outs[0]["planes"][0, 0, 2] == np.float32((11.0 - 0.125) / R.CFG["xy_scale"])      # slot 0's plane, not the nearer slot 2's
    assert outs[9]["planes"][0, 0, 2] == np.float32((11.0 - 13.625) / R.CFG["xy_scale"])
    wide = R.run(rec, poses, vel, **dict(R.CFG, planes=2))
    assert all(o["state"]["flags"][0] == 0 for o in wide) and wide[0]["planes"][0, 1, 2] == np.float32((9.0 - 0.125) / R.CFG["xy_scale"])
    # the probe passes x = 12 at step 10 (slot 2) and x = 14 at step 11 (slot 0): two runs, the first one's slot is kept
    last = _ints(outs[-1]["state"])
    assert last["red_runs"] == 2 and last["first_slot"] == 2 and last["first_tick"] == 10


def test_a_held_scene_keeps_its_record_and_shows_inert_planes_but_its_phases():
    rec, (poses, vel) = R.scenario_a()
    hold = np.zeros((24, 1), dtype=np.int32)
    hold[7:] = 1
    outs = R.run(rec, poses, vel, hold, **R.CFG)
    assert _emitting(outs) == [6]
    frozen = R.pack_state(outs[6]["state"])
    assert all(np.array_equal(R.pack_state(o["state"]), frozen) for o in outs[7:]) and _ints(outs[-1]["state"])["ticks"] == 6
    assert all((o["planes"] == np.array(R.INERT, dtype=np.float32)).all() for o in outs[7:])
    assert outs[7]["phase"].tolist() == [[3, 1, 3, 3]]            # written, for the time the step would have had: tick 7


def test_a_negative_offset_wraps_into_the_cycle():
    rec = R.from_lines([100.0, 0.0], 0.0, 4.0, R.LIGHT, 5.0, [-1.0, 2.0, 1.0, 5.0])[None, None]
    poses, vel = R.straight_drive(12)
    outs = R.run(rec, poses, vel, **R.CFG)
    # tau = -1 + 8 = 7 at t = 0, then -0.5 + 8, 0, 0.5, ...: red, red, four greens, two yellows, red
    assert [int(o["phase"][0, 0]) for o in outs] == [3, 3, 1, 1, 1, 1, 2, 2, 3, 3, 3, 3]


def test_every_kind_of_empty_slot_has_phase_zero_and_neither_binds_nor_counts():
    good = R.from_lines([12.0, 0.0], 0.0, 4.0, R.LIGHT, 20.0, [0.0, 0.0, 0.0, 1.0])
    sign = R.from_lines([12.0, 0.0], 0.0, 4.0, R.STOP, 20.0, [0.0, 0.0, 0.0, 0.0])
    edits = [(good, 4, 0.0), (good, 4, 3.0), (good, 4, np.nan), (good, 5, 0.0), (good, 5, -1.0), (good, 5, np.nan), (good, 7, -0.5),
             (good, 8, np.nan), (good, 9, -1.0), (good, 9, 0.0), (sign, 5, 0.0), (sign, 4, 1.5)]
    rec = np.zeros((1, len(edits) + 2, 10))
    for j, (base, col, val) in enumerate(edits):
        rec[0, j] = base
        rec[0, j, col] = val
    rec[0, len(edits)] = good
    rec[0, len(edits), 2:4] = good[0:2]                          # L = 0
    rec[0, len(edits) + 1] = sign
    rec[0, len(edits) + 1, 7:10] = [-1.0, np.nan, -5.0]          # a sign's timing is not read
    poses, vel = R.straight_drive(12)
    outs = R.run(rec, poses, vel, **dict(R.CFG, planes=8))
    assert all(o["phase"][0].tolist() == [0] * (len(edits) + 1) + [4] for o in outs)
    assert all(o["emit"][0].tolist() == [False] * (len(edits) + 1) + [t <= 7] for t, o in enumerate(outs))
    assert _ints(outs[-1]["state"]) == dict(ZERO, ticks=11, have=1, stop_runs=1, stops_met=1, first_tick=8, first_slot=len(edits) + 1)


def test_the_record_packs_as_the_contract_lays_it_out_and_reset_clears_masked_scenes():
    rec, (poses, vel) = R.scenario_a()
    st = R.run(rec, poses, vel, **R.CFG)[-1]["state"]
    w = R.pack_state(st)
    assert w.shape == (1, 16) and w.dtype == np.int32 and w[0, :12].tolist() == [23, 1, 0, 0, 1, 0, 0, 10, 0, 0, 0, 0]
    assert w.view(np.float64)[0, 6] == 32.625 and all(np.array_equal(v, R.unpack_state(w)[k]) for k, v in st.items())
    two = {k: np.concatenate([v, v]) for k, v in st.items()}
    cleared = R.reset(two, np.array([0, 1]))
    assert np.array_equal(R.pack_state(cleared)[0], w[0]) and not R.pack_state(cleared)[1].any()


# ---- the random drives the device is compared on -------------------------------------------------------------------------------------
def test_the_random_drives_stay_clear_of_every_threshold_and_contain_every_event():
    seen = dict(red=0, ran=0, completed=0, overflow=0, held=0)
    for S, N, P, T in [c + (R.STEPS,) for c in R.CASES] + [R.FREE]:
        d = R.random_drive(S, N, P, T)
        assert d["signals"].shape == (S, N, 10) and d["poses"].shape == (T, S, 3) and d["velocities"].dtype == np.float32
        assert np.nanmax(np.abs(d["signals"][..., :4])) < 300.0 and np.abs(d["poses"][..., :2]).max() < 300.0
        outs = R.run(d["signals"], d["poses"], d["velocities"], d["holds"], **d["cfg"])
        slack = min(o["slack"] for o in outs)
        assert slack >= 1e-9, (S, N, P, slack)
        for k in ("red", "ran", "completed", "overflow"):
            seen[k] += sum(int(o[k].sum()) for o in outs)
        seen["held"] += int(d["holds"].any(axis=0).sum())
        for o in outs:
            assert (o["planes_bound"] < 1e-6).all() and (np.abs(o["planes"][..., :2]) <= 1.0 + 1e-6).all()
    assert all(v >= 1 for v in seen.values()), seen
    # the drives that free-run and the largest one bring every event on their own
    d = R.random_drive(*R.FREE)
    outs = R.run(d["signals"], d["poses"], d["velocities"], d["holds"], **d["cfg"])
    assert all(sum(int(o[k].sum()) for o in outs) >= 1 for k in ("red", "ran", "completed", "overflow"))


def test_the_probe_bound_is_far_below_the_slack():
    d = R.random_drive(*R.FREE)
    assert R.qxy_bound(d["poses"][:, :, :2], -2.0).max() < 1e-12


# ---- the refusals, all before a launch ------------------------------------------------------------------------------------------------
def test_state_sizes_and_host_side_validation(built):
    L = built
    assert L.lazy("adx_signals_state_bytes")(3) == 192 and L.lazy("adx_signals_state_bytes")(0) == 0 == L.lazy("adx_signals_state_bytes")(65536)
    buf = (C.c_double * 512)()
    p = C.addressof(buf)
    good = dict(scenes=1, n_signals=2, n_planes=2, stop_on_yellow=0, dt=0.5, xy_scale=23.315, margin=3.0, probe=-2.0, min_cos=0.0,
                speed_threshold=0.1)
    args = lambda **kw: tuple(dict(dict(signals=p, pose=p + 256, velocity=p + 512, hold=None, state=p + 1024, planes=p + 2048,  # noqa: E731
                                        phase=p + 3072), **kw).values()) + (None,)
    step = L.lazy("adx_signals_step")
    for bad, text in ((dict(scenes=0), "0 scenes"), (dict(scenes=65536), "65536 scenes"), (dict(n_signals=0), "0 signals"),
                      (dict(n_signals=65), "65 signals"), (dict(n_planes=0), "0 planes"), (dict(n_planes=9), "9 planes"),
                      (dict(dt=0.0), "dt 0"), (dict(dt=float("nan")), "dt nan"), (dict(xy_scale=float("inf")), "xy_scale inf"),
                      (dict(margin=-1.0), "margin -1"), (dict(probe=float("inf")), "probe inf"), (dict(probe=float("nan")), "probe nan"),
                      (dict(min_cos=1.0), "min_cos 1"), (dict(min_cos=-1.5), "min_cos -1.5"), (dict(min_cos=float("nan")), "min_cos nan"),
                      (dict(speed_threshold=-0.1), "speed_threshold -0.1")):
        cfg = L.SignalsCfg(**dict(good, **bad))
        assert step(C.byref(cfg), *args()) == -1, bad
        assert text.encode() in L.lib().adx_last_error(), (bad, L.lib().adx_last_error())
    cfg = L.SignalsCfg(**good)
    assert step(None, *args()) == -1 and b"null configuration" in L.lib().adx_last_error()
    for name in ("signals", "pose", "velocity", "state", "planes", "phase"):
        assert step(C.byref(cfg), *args(**{name: None})) == -1
        assert f"null {name}".encode() in L.lib().adx_last_error(), (name, L.lib().adx_last_error())
    for kw, text in ((dict(state=p + 8), "the state aliases signals"), (dict(planes=p + 256), "planes aliases pose"),
                     (dict(phase=p + 512), "phase aliases velocity"), (dict(hold=p + 2048), "planes aliases hold"),
                     (dict(planes=p + 1024 + 32), "the state and planes alias each other"),
                     (dict(phase=p + 2048 + 20), "planes and phase alias each other"), (dict(phase=p + 1024), "the state and phase alias")):
        assert step(C.byref(cfg), *args(**kw)) == -1, kw
        assert text.encode() in L.lib().adx_last_error(), (kw, L.lib().adx_last_error())
    reset = L.lazy("adx_signals_reset")
    for a, text in (((None, 1, None, None, 0), "null state"), ((p, 0, None, None, 0), "0 scenes"), ((p, 1, None, p + 256, 9), "9 planes"),
                    ((p, 1, p + 8, None, 0), "the mask overlaps the state"), ((p, 1, None, p + 32, 2), "planes_out overlaps the state"),
                    ((p, 1, p + 256, p + 256, 2), "the mask overlaps planes_out")):
        assert reset(*a, None) == -1 and text.encode() in L.lib().adx_last_error(), (a, L.lib().adx_last_error())


def test_signals_refuse_before_a_launch(built):
    from autonomous_driving_with_diffusion_model_amd import Signals
    from autonomous_driving_with_diffusion_model_amd.simulation import World
    rec, _ = R.scenario_a()
    rec = np.concatenate([rec, rec])                              # S = 2
    kw = dict(dt=0.5, xy_scale=23.315)
    for bad, err, text in ((dict(planes=0), ValueError, "planes must be 1..8"), (dict(planes=9), ValueError, "planes must be 1..8"),
                           (dict(dt=0.0), ValueError, "dt must be finite and > 0"), (dict(xy_scale=float("nan")), ValueError, "xy_scale"),
                           (dict(margin=-1.0), ValueError, "margin must be finite and >= 0"), (dict(probe=float("inf")), ValueError, "probe must be finite"),
                           (dict(probe=float("nan")), ValueError, "probe must be finite"), (dict(min_cos=1.0), ValueError, r"min_cos must lie in \[-1, 1\)"),
                           (dict(min_cos=float("nan")), ValueError, "min_cos"), (dict(speed_threshold=float("inf")), ValueError, "speed_threshold")):
        with pytest.raises(err, match=text):
            Signals(rec, **dict(kw, **bad))
    with pytest.raises(TypeError, match="records must be float64"):
        Signals(torch.zeros(2, 4, 10), **kw)
    with pytest.raises(ValueError, match=r"records must be \[S, N, 10\]"):
        Signals(np.zeros((2, 4, 9)), **kw)
    with pytest.raises(ValueError, match=r"records must be \[S, N, 10\]"):
        Signals(np.zeros((4, 10)), **kw)
    with pytest.raises(ValueError, match="signals per scene must be 1..64"):
        Signals(np.zeros((2, 65, 10)), **kw)
    with pytest.raises(ValueError, match="signals per scene must be 1..64"):
        Signals(np.zeros((2, 0, 10)), **kw)
    with pytest.raises(ValueError, match="scenes must be 1..65535"):
        Signals(np.zeros((0, 4, 10)), **kw)
    sig = Signals(rec, **kw)
    assert sig.device.type == "cpu" and sig.state.shape == (2, 16) and sig.phase.shape == (2, 4) and sig.planes.shape == (2, 4, 3)
    assert sig.planes.tolist() == [[[0.0, 0.0, 1.0]] * 4] * 2 and not sig.primed and not sig.state.any()
    assert sig.key() != Signals(rec, **dict(kw, margin=2.0)).key() and "planes=4" in repr(sig)
    rec[0, 0, 0] = 99.0
    assert sig.records[0, 0, 0].item() == 12.0                   # host values are copied
    pose, vel = torch.zeros(2, 3, dtype=torch.float64), torch.zeros(2)
    for a, text in (((pose.float(), vel), "pose must be contiguous torch.float64"), ((torch.zeros(3, 3, dtype=torch.float64), vel), "pose must be"),
                    ((pose, vel.double()), "velocity must be contiguous torch.float32"), ((pose, torch.zeros(3)), "velocity must be"),
                    (([[0.0] * 3] * 2, vel), "pose must be")):
        with pytest.raises(ValueError, match=text):
            sig.step(*a)
    with pytest.raises(ValueError, match="hold must be contiguous torch.int32"):
        sig.step(pose, vel, hold=torch.zeros(2))
    with pytest.raises(ValueError, match=r"mask must be \[2\] bool or uint8"):
        sig.reset(torch.zeros(2))
    with pytest.raises(built.AdxError, match="there is no CPU path"):
        sig.step(pose, vel)
    with pytest.raises(built.AdxError, match="there is no CPU path"):
        sig.reset()
    with pytest.raises(ValueError, match="not a snapshot"):
        sig.state_restore(torch.zeros(2, 15, dtype=torch.int32))
    assert not sig.primed and not sig.state.any()
    # compute and fields read the record as the restatement packs it
    rec_a, (poses, v) = R.scenario_a()
    st = R.run(rec_a, poses, v, **R.CFG)[-1]["state"]
    sig.state[0] = torch.from_numpy(R.pack_state(st)[0])
    sig.state[1, 5], sig.state[1, 4], sig.state[1, 10] = 2, 1, 1
    out = sig.compute()
    assert out["red_runs"].tolist() == [1, 1] and out["stop_runs"].tolist() == [0, 2] and out["first_tick"].tolist() == [10, 0]
    assert out["overflow"].tolist() == [False, True] and out["penalty"] == pytest.approx([0.7, 0.448], rel=1e-14) and out["ticks"].tolist() == [23, 0]
    f = Signals.fields(sig.words())
    assert f["qx"][0] == 32.625 and set(f) == set(R.INTS + R.F64)
    # from_lines is the contract's construction
    mine = Signals.from_lines([[12.0, 0.0], [3.0, 4.0]], [0.0, 1.1], 4.0, [1.0, 2.0], 20.0, [0.5, 2.0, 1.0, 5.0])
    assert mine.dtype == torch.float64 and np.array_equal(mine.numpy(), R.from_lines([[12.0, 0.0], [3.0, 4.0]], [0.0, 1.1], 4.0, [1.0, 2.0], 20.0,
                                                                                     [0.5, 2.0, 1.0, 5.0]))
    assert mine[0, :4].tolist() == [12.0, 2.0, 12.0, -2.0]
    # the world checks its signals against the rest
    with pytest.raises(TypeError, match="signals must be a Signals"):
        World(signals=rec)
    with pytest.raises(ValueError, match="one scene count, one device"):
        World(discs=torch.zeros(3, 1, 5, dtype=torch.float64), signals=sig)
    w = World(signals=sig)
    assert w.signals is sig and w.discs is None and World().signals is None
    w.advance(0.5)
