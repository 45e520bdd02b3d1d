"""CPU: the one declaration of a guide's records (guide.py, RECORDS) and what walks it, without a device and without the library --
the key and `descs` rule over all 16 subsets of records, every agreement refusal of `Guide.__init__` by its whole text (the
expected texts are literals here, not built from the package's table), `clone`, `copy_`, and the 25 generated ctypes signatures of
the guided exports against their declarations in include/adx.h."""
import ctypes as C
import itertools
import os
import re

import pytest
import torch

from autonomous_driving_with_diffusion_model_amd import _lib as L
from autonomous_driving_with_diffusion_model_amd.guide import Capsules, CostField, Guide, MotionLimits, Route

S = 2
ATTRS = ("field", "motion", "route", "capsules")
SUFFIXES = ("guide", "field", "motion", "route", "capsule")
STRUCTS = (L.GuideDesc, L.FieldDesc, L.MotionDesc, L.RouteDesc, L.CapsuleDesc)
V1 = (1, 0, 0.5, "constant", 0.25, 2)


def _make(what: str, scenes: int = S, device: str = "cpu", fill: float = 0.0):
    """One constraint of a guide by the keyword `Guide` takes it under: the smallest tensors each constructor accepts."""
    full = lambda *shape: torch.full(shape, fill, device=device)  # noqa: E731
    if what == "discs":
        return full(scenes, 1, 5)
    if what == "planes":
        return full(scenes, 1, 3)
    if what == "field":
        return CostField(full(scenes, 2, 3), (0.5, -1.0), (0.25, 0.5), 2.0)
    if what == "motion":
        return MotionLimits(full(scenes, 2), 1.5, 2.5)
    if what == "route":
        return Route(full(scenes, 4, 2), full(scenes), 3.0)
    return Capsules(full(scenes, 3, 7), 0.75)


def _subsets():
    return [tuple(a for a, on in zip(ATTRS, bits) if on) for bits in itertools.product((False, True), repeat=4)]


def _guide(held, **kw):
    return Guide(_make("discs"), None, 0.5, "constant", 0.25, 2, **{a: _make(a, **kw) for a in held})


@pytest.mark.parametrize("held", _subsets(), ids=lambda h: "+".join(h) or "v1")
def test_key_and_descs_run_through_the_last_record_held(held, monkeypatch):
    """`key()`: the v1 6-tuple, then each record's own `key()` through the last one held, None for an absent one in between.
    `descs()`: the suffix of the last one held ("guide" with none), a reference per record through that one with None in the same
    places, and the structs those references point at."""
    guide = _guide(held)
    records = [getattr(guide, a) for a in ATTRS]
    last = max((i for i, r in enumerate(records) if r is not None), default=-1)
    assert guide.records() == tuple(records)
    assert guide.key() == V1 + tuple(None if r is None else r.key() for r in records[:last + 1])
    assert len(guide.key()) == 6 + last + 1 and (last < 0 or guide.key()[-1] is not None)
    monkeypatch.setattr(L, "require_gpu_f32", lambda t, name, dtype=torch.float32: t)      # `descs` launches nothing
    suffix, refs, structs = guide.descs(torch.zeros(2 * S, 8, 4), 0.05)
    assert suffix == SUFFIXES[last + 1]
    assert [r is None for r in refs] == [s is None for s in structs] == [False] + [r is None for r in records[:last + 1]]
    for ref, struct, kind in zip(refs, structs, STRUCTS):
        assert struct is None or (type(struct) is kind and C.addressof(ref._obj) == C.addressof(struct))
    assert structs[0].lambda_ == C.c_float(0.05).value and structs[0].discs == guide.discs.data_ptr()
    for struct, record in zip(structs[1:], records):
        assert struct is None or (struct.scene_rows == S and getattr(struct, type(struct)._fields_[0][0]) == record.lead.data_ptr())


# (keyword of the later record, what a refusal calls it, [(keyword of an earlier entry, what a refusal calls that one)])
AGREEMENTS = (
    ("field", "the field", (("discs", "discs"), ("planes", "planes"))),
    ("motion", "the motion limits", (("discs", "discs"), ("planes", "planes"), ("field", "field"))),
    ("route", "the route", (("discs", "discs"), ("planes", "planes"), ("field", "field"), ("motion", "motion limits"))),
    ("capsules", "the capsules", (("discs", "discs"), ("planes", "planes"), ("field", "field"), ("motion", "motion limits"),
                                  ("route", "route"))),
)
PAIRS = [(later, noun, earlier, name) for later, noun, before in AGREEMENTS for earlier, name in before]


def test_there_are_fourteen_pairs():
    assert len(PAIRS) == 2 + 3 + 4 + 5 == 14


@pytest.mark.parametrize("later, noun, earlier, name", PAIRS, ids=[f"{p[2]}-{p[0]}" for p in PAIRS])
def test_a_record_agrees_with_every_entry_before_it(later, noun, earlier, name):
    """Scenes and device of each (earlier, later) pair, by the whole text of the refusal; the device is asked first."""
    with pytest.raises(ValueError) as e:
        Guide(**{earlier: _make(earlier, 2), later: _make(later, 3)})
    assert str(e.value) == f"Guide: {name} hold 2 scenes, {noun} 3"
    with pytest.raises(ValueError) as e:
        Guide(**{earlier: _make(earlier, 2, "meta"), later: _make(later, 2)})
    assert str(e.value) == f"Guide: {name} live on meta, {noun} on cpu"
    with pytest.raises(ValueError) as e:
        Guide(**{earlier: _make(earlier, 2, "meta"), later: _make(later, 3)})
    assert str(e.value) == f"Guide: {name} live on meta, {noun} on cpu"
    assert Guide(**{earlier: _make(earlier), later: _make(later)}).scenes == S


@pytest.mark.parametrize("later", ATTRS)
def test_discs_and_planes_without_a_constraint_agree_with_everything(later):
    guide = Guide(torch.zeros(3, 0, 5), torch.zeros(3, 0, 3), **{later: _make(later)})
    assert (guide.scenes, guide.M, guide.P) == (3, 0, 0) and getattr(guide, later).scenes == S


def test_a_record_of_another_kind_is_refused_by_name():
    for attr, kind, other in (("field", "CostField", "motion"), ("motion", "MotionLimits", "route"), ("route", "Route", "capsules"),
                              ("capsules", "Capsules", "field")):
        with pytest.raises(TypeError) as e:
            Guide(**{attr: _make(other)})
        assert str(e.value) == f"Guide: {attr} must be a {kind} or None, got {type(_make(other)).__name__}"


NAMES = ("discs", "planes", "field.cells", "motion.limits", "route.points", "route.half_width", "capsules.slots")


def _full(fill: float, discs="tensor"):
    d = {"tensor": _make("discs", fill=fill), "none": None, "empty": torch.zeros(S, 0, 5)}[discs]
    return Guide(d, _make("planes", fill=fill), 0.5, "constant", 0.25, 2, **{a: _make(a, fill=fill) for a in ATTRS})


def test_tensors_names_every_tensor_in_order():
    guide = _full(1.0)
    assert tuple(n for n, _ in guide.tensors()) == NAMES
    assert [t.data_ptr() for _, t in guide.tensors()] == [t.data_ptr() for t in (
        guide.discs, guide.planes, guide.field.cells, guide.motion.limits, guide.route.points, guide.route.half_width,
        guide.capsules.slots)]
    assert tuple(n for n, _ in Guide(route=_make("route")).tensors()) == ("route.points", "route.half_width")
    assert Guide().tensors() == () and Guide().scenes is None and Guide().device is None
    for attr, name in zip(ATTRS, ("field.cells", "motion.limits", "route.points", "capsules.slots")):
        guide = Guide(**{attr: _make(attr, 3)})              # the first tensor says how many scenes and where
        assert guide.scenes == 3 and guide.device == torch.device("cpu") and guide.tensors()[0][0] == name


@pytest.mark.parametrize("held", _subsets(), ids=lambda h: "+".join(h) or "v1")
def test_clone_gives_an_equal_guide_over_storage_of_its_own(held):
    guide = _guide(held, fill=1.25)
    twin = guide.clone()
    assert twin.key() == guide.key() and repr(twin) == repr(guide)
    assert [n for n, _ in twin.tensors()] == [n for n, _ in guide.tensors()] and len(guide.tensors()) >= 1
    for (_, a), (_, b) in zip(guide.tensors(), twin.tensors()):
        assert torch.equal(a, b) and a.shape == b.shape and a.data_ptr() != b.data_ptr()
    for a, b in zip(guide.records(), twin.records()):
        assert (a is None) == (b is None) and (a is None or (type(a) is type(b) and a is not b))


def test_copy_moves_every_value_and_keeps_the_key():
    dst, src = _full(0.0), _full(1.5)
    key, pointers = dst.key(), [t.data_ptr() for _, t in dst.tensors()]
    assert dst.copy_(src) is dst
    assert dst.key() == key and [t.data_ptr() for _, t in dst.tensors()] == pointers
    assert len(dst.tensors()) == 7 and all(bool((t == 1.5).all()) for _, t in dst.tensors())
    assert all(bool((t == 1.5).all()) for _, t in src.tensors())


@pytest.mark.parametrize("dst_discs, src_discs", (("none", "empty"), ("empty", "none")))
def test_copy_between_no_discs_and_empty_discs(dst_discs, src_discs):
    """Two guides of equal key may differ in whether `discs` is None or an empty [S, 0, 5]: M is 0 either way."""
    dst, src = _full(0.0, dst_discs), _full(2.5, src_discs)
    assert dst.key() == src.key() and dst.M == src.M == 0
    key = dst.key()
    dst.copy_(src)
    assert dst.key() == key and (dst.discs is None) == (dst_discs == "none")
    named = dict(dst.tensors())
    assert set(named) - {"discs"} == set(NAMES[1:]) and all(bool((named[n] == 2.5).all()) for n in NAMES[1:])


def test_copy_refuses_a_guide_of_another_key():
    with pytest.raises(ValueError, match="Guide.copy_: the keys differ"):
        _guide(("field",)).copy_(_guide(("field", "route")))


def test_pointwise_records_are_the_ones_the_stop_short_export_takes():
    guide = _full(0.0)
    assert guide.pointwise() == (guide.field, guide.route, guide.capsules)
    assert Guide(motion=_make("motion")).pointwise() == (None, None, None)


# ---- the generated signatures against the header ----------------------------------------------------------------------------------
HEADER_STRUCTS = {"adx_step_coef": L.StepCoef, "adx_dpm_coef": L.DpmCoef, "adx_pin": L.PinDesc, "adx_guide": L.GuideDesc,
                  "adx_guide_field": L.FieldDesc, "adx_guide_motion": L.MotionDesc, "adx_guide_route": L.RouteDesc,
                  "adx_guide_capsules": L.CapsuleDesc, "adx_select_guide_cfg": L.SelectGuideCfg}
GUIDED = [f"adx_{step}_step_{suffix}" for suffix in SUFFIXES for step in ("ddim", "ddpm", "dpm")] + \
         [family + ("" if suffix == "guide" else "_" + suffix) for suffix in SUFFIXES for family in ("adx_guide_cost", "adx_traj_select_guide")]


def _ctype(c_type: str):
    """The ctypes type of one C parameter type of include/adx.h."""
    struct = re.fullmatch(r"const (adx_\w+)\*", c_type)
    if struct and struct.group(1) in HEADER_STRUCTS:
        return C.POINTER(HEADER_STRUCTS[struct.group(1)])
    if c_type.endswith("*") or c_type == "adx_stream":
        return L.vp
    return {"int32_t": L.i32, "int64_t": L.i64}[c_type]           # anything else: a KeyError, the map does not know it


@pytest.fixture(scope="module")
def header():
    with open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "adx.h")) as fh:
        return fh.read()


def test_there_are_twenty_five_guided_exports():
    assert len(GUIDED) == len(set(GUIDED)) == 25 and set(GUIDED) <= set(L._LAZY_SIGS) and set(GUIDED) <= set(L.EXPORTED_SYMBOLS)


@pytest.mark.parametrize("name", GUIDED)
def test_a_generated_signature_is_the_headers_declaration(name, header):
    found = re.findall(r"^int\s+" + name + r"\s*\(([^)]*)\)\s*;", header, re.M)
    assert len(found) == 1, name
    params = [" ".join(p.split()) for p in found[0].split(",")]
    types = [re.fullmatch(r"(.*?)\s*\b\w+", p).group(1).replace(" *", "*") for p in params]      # drop the parameter's name
    result, args = L._LAZY_SIGS[name]
    assert result is L.i32 and list(args) == [_ctype(t) for t in types], (name, types)
    assert len(args) == len(params)
