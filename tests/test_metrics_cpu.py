"""CPU: "open-loop metrics v1" -- every refusal of adx_traj_metrics, adx_metrics_accumulate and adx_metrics_reset by its whole
text, on the host before any GPU work; the four ctypes signatures and the struct against their declarations in include/adx.h;
the fp64 restatement (tests/metrics_ref.py) against a brute-force loop version; the margins of the shared construction; the host
accumulation against plain sums; OpenLoopMetrics refusing CPU tensors."""
import ctypes
import math
import os
import re

import numpy as np
import pytest
import torch

import metrics_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def built():
    import __graft_entry__ as g
    g.build()
    from autonomous_driving_with_diffusion_model_amd import _lib
    return _lib


def _declaration(header: str, name: str):
    m = re.search(r"^(\w+)\s+" + name + r"\s*\(([^)]*)\)\s*;", header, re.M)
    assert m, name
    args = [a.strip() for a in m.group(2).replace("\n", " ").split(",")]
    return m.group(1), [] if args == ["void"] else args


def test_signatures_and_struct_match_the_header(built):
    header = open(os.path.join(ROOT, "include", "adx.h")).read()
    assert "Open-loop metrics v1" in header

    def ctype(decl: str):
        if "adx_metrics_cfg*" in decl:
            return ctypes.POINTER(built.MetricsCfg)
        if "*" in decl or decl.startswith("adx_stream"):
            return ctypes.c_void_p
        return {"int32_t": ctypes.c_int32, "float": ctypes.c_float, "int": ctypes.c_int32, "size_t": ctypes.c_size_t}[decl.split()[0]]

    handle = ctypes.CDLL(built.LIB_PATH)
    for name, n_args in (("adx_traj_metrics", 12), ("adx_metrics_state_bytes", 0), ("adx_metrics_reset", 2), ("adx_metrics_accumulate", 10)):
        ret, args = _declaration(header, name)
        fn = getattr(built.lib(), name)
        assert hasattr(handle, name) and name in built.EXPORTED_SYMBOLS, name
        assert len(args) == n_args and list(fn.argtypes) == [ctype(a) for a in args], (name, args)
        assert fn.restype is ctype(ret), name
    body = re.search(r"typedef struct adx_metrics_cfg \{(.*?)\} adx_metrics_cfg;", header, re.S).group(1)
    declared = []
    for line in body.split(";"):
        line = line.strip()
        if line:
            kind, names = line.split(None, 1)
            declared += [(n.strip(), ctype(kind)) for n in names.split(",")]
    assert declared == list(built.MetricsCfg._fields_) and ctypes.sizeof(built.MetricsCfg) == 28
    assert built.lib().adx_metrics_state_bytes() == 8 * R.WORDS > 0


def test_every_refusal_by_its_whole_text_without_a_gpu(built):
    """The checks run on the host before any launch, so placeholder addresses (never dereferenced) are enough."""
    lib = built.lib()
    names = ("trajs", "gt", "valid", "index", "ade", "fde", "best", "rec", "flags", "disp_sel")
    base = {n: 0x10000000 * (k + 1) for k, n in enumerate(names)}
    S, K, H, D = 4, 3, 16, 7
    size = dict(trajs=K * S * H * D * 4, gt=S * H * 2 * 4, valid=S * 4, index=S * 4, ade=S * K * 4, fde=S * K * 4, best=S * 4, rec=S * 32,
                flags=S * 4, disp_sel=S * H * 4)

    def call(null_cfg=False, **kw):
        v = dict(scenes=S, candidates=K, horizon=H, dim=D, h0=1, miss_radius=2.0, xy_scale=23.315, **base)
        v.update(kw)
        c = built.MetricsCfg(v["scenes"], v["candidates"], v["horizon"], v["dim"], v["h0"], v["miss_radius"], v["xy_scale"])
        rc = lib.adx_traj_metrics(None if null_cfg else ctypes.byref(c), *(v[n] for n in names), None)
        return rc, lib.adx_last_error().decode()

    cases = [(dict(null_cfg=True), "traj metrics: null configuration"),
             (dict(candidates=0), "traj metrics: 0 candidates, supported 1..64"),
             (dict(candidates=65), "traj metrics: 65 candidates, supported 1..64"),
             (dict(horizon=0), "traj metrics: horizon 0, supported 1..64"),
             (dict(horizon=65), "traj metrics: horizon 65, supported 1..64"),
             (dict(dim=1), "traj metrics: the metrics score (x, y), dim is 1"),
             (dict(dim=0), "traj metrics: the metrics score (x, y), dim is 0"),
             (dict(scenes=0), "traj metrics: 0 scenes, supported 1..65535"),
             (dict(scenes=65536), "traj metrics: 65536 scenes, supported 1..65535"),
             (dict(scenes=65535, candidates=64, horizon=64, dim=16),
              "traj metrics: 4294901760 elements do not fit the kernel's 32-bit index"),
             (dict(h0=-1), "traj metrics: first scored waypoint -1, supported 0..15 (horizon 16)"),
             (dict(h0=16), "traj metrics: first scored waypoint 16, supported 0..15 (horizon 16)"),
             (dict(xy_scale=0.0), "traj metrics: xy_scale must be finite and > 0, got 0"),
             (dict(xy_scale=-1.5), "traj metrics: xy_scale must be finite and > 0, got -1.5"),
             (dict(xy_scale=math.inf), "traj metrics: xy_scale must be finite and > 0, got inf"),
             (dict(miss_radius=-0.5), "traj metrics: miss_radius must be >= 0, got -0.5"),
             (dict(trajs=None), "traj metrics: null input"), (dict(gt=None), "traj metrics: null input")]
    cases += [({n: None}, "traj metrics: null output") for n in names[4:]]
    # an output against every input (first byte, last byte, from below), and against every other output
    for o in names[4:]:
        for i in names[:4]:
            cases.append(({o: base[i]}, "traj metrics: an output overlaps an input"))
            cases.append(({o: base[i] + size[i] - 4}, "traj metrics: an output overlaps an input"))
            cases.append(({o: base[i] - size[o] + 4}, "traj metrics: an output overlaps an input"))
        for p in names[4:]:
            if p != o:
                cases.append(({o: base[p] + size[p] - 4}, "traj metrics: outputs overlap each other"))
    for kw, text in cases:
        rc, got = call(**kw)
        assert rc == -1 and got == text, (kw, got)
    for kw, head in ((dict(xy_scale=math.nan), "traj metrics: xy_scale must be finite and > 0, got "),
                     (dict(miss_radius=math.nan), "traj metrics: miss_radius must be >= 0, got ")):
        rc, got = call(**kw)
        assert rc == -1 and got.startswith(head) and got[len(head):].lstrip("-") == "nan", (kw, got)
    with pytest.raises(ValueError, match=r"^adx_traj_metrics: traj metrics: 65 candidates, supported 1\.\.64$"):
        built.check(call(candidates=65)[0], "adx_traj_metrics")

    # the accumulation and the reset
    an = ("state", "rec", "flags", "best", "index", "disp_sel", "blocked")
    ab = {n: 0x10000000 * (k + 1) for k, n in enumerate(an)}
    asize = dict(rec=S * 32, flags=S * 4, best=S * 4, index=S * 4, disp_sel=S * H * 4, blocked=S * 4)

    def acc(scenes=S, horizon=H, **kw):
        v = dict(ab)
        v.update(kw)
        rc = lib.adx_metrics_accumulate(*(v[n] for n in an), scenes, horizon, None)
        return rc, lib.adx_last_error().decode()

    cases = [(dict(scenes=0), "metrics accumulate: 0 scenes, supported 1..65535"),
             (dict(scenes=65536), "metrics accumulate: 65536 scenes, supported 1..65535"),
             (dict(horizon=0), "metrics accumulate: horizon 0, supported 1..64"),
             (dict(horizon=65), "metrics accumulate: horizon 65, supported 1..64"),
             (dict(state=None), "metrics accumulate: null state")]
    cases += [({n: None}, "metrics accumulate: null input") for n in ("rec", "flags", "best", "disp_sel")]
    for n in an[1:]:
        cases.append((dict(state=ab[n] + asize[n] - 4), "metrics accumulate: the state overlaps an input"))
        cases.append((dict(state=ab[n] - 8 * R.WORDS + 4), "metrics accumulate: the state overlaps an input"))
    for kw, text in cases:
        rc, got = acc(**kw)
        assert rc == -1 and got == text, (kw, got)
    assert lib.adx_metrics_reset(None, None) == -1 and lib.adx_last_error().decode() == "metrics reset: null state"


def test_open_loop_metrics_refuses_cpu_tensors_and_bad_shapes(built):
    import autonomous_driving_with_diffusion_model_amd as pkg
    from autonomous_driving_with_diffusion_model_amd.evaluation import OpenLoopMetrics, evaluate_open_loop
    assert pkg.OpenLoopMetrics is OpenLoopMetrics and pkg.evaluate_open_loop is evaluate_open_loop
    assert {"OpenLoopMetrics", "evaluate_open_loop", "MetricsBatch"} <= set(pkg.__all__)
    m = OpenLoopMetrics()
    assert (m.h0, m.miss_radius, m.xy_scale) == (1, 2.0, 23.315)
    with pytest.raises(built.AdxError, match="gt lives on cpu"):
        m.update(torch.zeros(6, 16, 7), torch.zeros(2, 16, 2))
    meta = lambda *shape, dtype=torch.float32: torch.zeros(*shape, dtype=dtype, device="meta")      # noqa: E731
    with pytest.raises(built.AdxError, match="lives on meta"):
        m.update(meta(6, 16, 7), meta(2, 16, 2))
    assert m.state is None
    empty = m.compute()                                     # nothing seen: counts of zero, averages over nothing
    assert empty["n"] == 0 and empty["nonfinite"] == 0 and math.isnan(empty["ade"]) and empty["disp_at"] == []
    assert empty["units"] == {"distance": "m", "xy_scale": 23.315, "miss_radius_m": 2.0, "h0": 1}
    with pytest.raises(ValueError, match="candidates must be 1..64"):
        evaluate_open_loop(None, None, None, [], candidates=65)


@pytest.mark.parametrize("S,K,H,D", R.SHAPES)
@pytest.mark.parametrize("h0", [0, 1])
def test_restatement_against_the_loop_version(S, K, H, D, h0):
    """Full, ragged and degenerate inputs: a valid vector with 0, h0, h0 + 1 and values beyond both ends, indices in and out of
    range, a NaN and an infinite waypoint, two equal rows, a zero-length last segment."""
    trajs, gt, _ = R.case(S, K, H, D, seed=3)
    rng = np.random.default_rng(S * 100 + K)
    for variant in range(4):
        t, g = trajs.copy().reshape(K, S, H, D), gt.copy()
        valid = index = None
        if variant >= 1:
            valid = np.array([(0, h0, h0 + 1, H, H + 3, -2, max(h0 + 2, H // 2))[(s + variant) % 7] for s in range(S)])
            index = rng.integers(-1, K + 1, size=S)
        if variant >= 2:
            t[rng.integers(K), rng.integers(S), rng.integers(H), rng.integers(2)] = np.nan
            t[rng.integers(K), rng.integers(S), rng.integers(H), rng.integers(2)] = np.inf
            if K > 1:
                t[1] = t[0]
        if variant == 3 and H >= 2:
            g[:, -1] = g[:, -2]
            valid = None
        a = R.metrics(t, g, valid, index, h0)
        ade, fde, best, rec, flags, disp = R.metrics_loops(t, g, valid, index, h0)
        kw = dict(rtol=1e-13, atol=0, equal_nan=True)
        assert np.allclose(a.ade, ade, **kw) and np.allclose(a.fde, fde, **kw) and np.allclose(a.disp_sel, disp, **kw)
        assert np.allclose(a.rec, rec, rtol=1e-12, atol=1e-15, equal_nan=True)
        assert a.best.tolist() == best and a.flags.tolist() == flags, variant
        if variant == 3 and H >= 2:
            assert not (a.flags & R.HEADING).any() and not a.rec[:, 4:6].any()


def test_the_search_rule():
    inf, nan = np.inf, np.nan
    for v, want in (([3.0, 1.0, 1.0], 1), ([nan, 2.0], 1), ([inf, nan], 0), ([nan], 0), ([inf, 5.0, -inf, 4.0], 3), ([2.0, 2.0], 0)):
        assert R.argmin_finite(v) == want, v


def test_the_construction_decides_every_scene_by_more_than_rounding():
    """The inputs of tests/test_gpu_metrics.py: at (64, 64, 64) neighbouring candidates' ADE and FDE differ by at least 0.18 m,
    every FDE keeps clear of the 2.0 m radius, and the arg-min is the candidate with p = 0 in every scene; at every shape of the
    GPU test, with h0 = 0 and 1, every margin exceeds twice the bound -- checked here, where no GPU is needed."""
    trajs, gt, p = R.case(64, 64, 64, 2)
    ref = R.metrics(trajs, gt, h0=1)
    order = np.argsort(p, axis=1)
    for v in (ref.ade, ref.fde):
        ranked = np.take_along_axis(v, order, axis=1)
        assert np.diff(ranked, axis=1).min() >= 0.18
    assert np.abs(ref.fde - 2.0).min() >= 0.045 and ref.ade.max() < 12.1
    assert np.array_equal(ref.best, order[:, 0]) and (ref.flags & 7 == 7).all()
    worst = 0.0
    for S, K, H, D in R.SHAPES:
        for h0 in (0, 1):
            trajs, gt, _ = R.case(S, K, H, D)
            ref = R.metrics(trajs, gt, h0=h0)
            b = R.bound(ref, h0)
            assert (b.ade <= 64 * R.gamma(71) * 12.1).all()          # the bound is a few 1e-5 m at most: not a tolerance in disguise
            for s, m in R.margins(ref, b):
                for name, (margin, allowed) in m.items():
                    assert margin > 2 * allowed, (S, K, H, D, h0, s, name, margin, allowed)
                    worst = max(worst, allowed)
    print(f"largest allowed rounding at a decision: {worst:.3e} m")


def test_host_accumulation_is_the_plain_sums():
    trajs, gt, _ = R.case(5, 7, 24, 3)
    trajs = trajs.reshape(7, 5, 24, 3)
    trajs[2, 1, 5, 0] = np.nan
    index = np.array([0, 2, 6, 7, 3])                 # scene 1 chooses the NaN candidate, scene 3 is out of range
    valid = np.array([24, 24, 10, 24, 1])             # scene 4: nothing to score at h0 = 1
    blocked = np.array([1, 1, 0, 1, 1])
    ref = R.metrics(trajs, gt, valid, index, h0=1)
    rec32, disp32 = ref.rec.astype(np.float32), ref.disp_sel.astype(np.float32)
    counts, sums = R.accumulate(*R.fresh_state(), rec32, ref.flags, ref.best, index, disp32, blocked, 24)
    assert ref.flags.tolist()[3:] == [0, 0] and not ref.flags[1] & R.FINITE
    assert counts[R.W_SCORED] == 3 and counts[R.W_NONFINITE] == 1 and counts[R.W_BLOCKED] == 1 and counts[R.W_HEADING] == 2
    used = [0, 2]
    assert sums[R.W_REC + 2] == float(np.float64(rec32[0, 2]) + np.float64(rec32[2, 2]))
    assert counts[R.W_DISP_COUNT:R.W_DISP_COUNT + 24].tolist() == [0] + [2] * 9 + [1] * 14
    assert np.isfinite(sums).all() and sums[R.W_REGRET] >= 0
    out = R.summary(counts, sums, 24)
    assert out["n"] == 2 and out["min_ade_k"] <= out["ade"] and out["blocked_rate"] == 0.5
    assert out["ade"] == pytest.approx(np.mean(ref.rec[used, 2]), rel=1e-6)


def test_the_eval_tool_parses_its_variants_and_prints_strict_json():
    import json
    import sys
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import open_loop_eval as T
    assert T.parse_variant("dpm:10:8:0") == ("dpm", 10, 8, 0) and T.parse_variant("ddim:50:1:10") == ("ddim", 50, 1, 10)
    for bad in ("ddim:50:1", "euler:10:1:0", "ddim:50:1:0:0"):
        with pytest.raises(SystemExit, match="scheduler:steps:candidates:warm_steps"):
            T.parse_variant(bad)
    line = json.dumps(T._strict({"ade": 1.5, "disp_at": [float("nan"), 2.0], "units": {"h0": 1}, "n": 3}), allow_nan=False)
    assert json.loads(line) == {"ade": 1.5, "disp_at": [None, 2.0], "units": {"h0": 1}, "n": 3}
