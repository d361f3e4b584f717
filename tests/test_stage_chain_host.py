"""The stage chain of inference.py and the validator of its stage dicts, on the CPU: ``_run_stages`` runs first -> stage 1 ->
stage 2, hands the reference to the last call alone and returns that call's tallies; ``postprocess.check_stage_kwargs`` takes
every key of the four key tuples and refuses a bad dict with a ValueError that names the argument."""
import itertools

import pytest
import torch

from diff_unet_amos_amd import inference, postprocess

STAGES, FORMS = ("postprocess", "fill_holes"), ("mask", "map")
KEYS = {("postprocess", "mask"): inference.POSTPROCESS_KEYS, ("postprocess", "map"): inference.SEGMENT_POSTPROCESS_KEYS,
        ("fill_holes", "mask"): postprocess.FILL_HOLES_KEYS, ("fill_holes", "map"): postprocess.FILL_HOLES_MAP_KEYS}
GOOD = dict(connectivity=2, num_components=3, min_size=10, cap=64, channels=(1, 2), classes=[1, 2])


def _chain(n_stages, reference):
    """_run_stages over stubs: (what it returned, the log of (name, result it was given, reference it saw))."""
    log = []

    def first(ref):
        log.append(("first", None, ref))
        return "r0", "t0" if ref is not None else None

    def stage(i):
        def run(result, ref):
            log.append((f"stage{i}", result, ref))
            return f"r{i}", f"t{i}" if ref is not None else None
        return run

    return inference._run_stages(first, [stage(i) for i in range(1, n_stages + 1)], reference), log


@pytest.mark.parametrize("n_stages", [0, 1, 2])
@pytest.mark.parametrize("reference", [None, "ref"])
def test_run_stages_runs_in_order_and_only_the_last_call_sees_the_reference(n_stages, reference):
    (result, tallies), log = _chain(n_stages, reference)
    assert [name for name, _, _ in log] == ["first", "stage1", "stage2"][:n_stages + 1]
    assert [given for _, given, _ in log] == [None, "r0", "r1"][:n_stages + 1]           # each stage gets the result before it
    assert [ref for _, _, ref in log] == [None] * n_stages + [reference]                 # exactly one call, the last, sees it
    assert result == f"r{n_stages}"
    assert tallies == (None if reference is None else f"t{n_stages}")                    # the tallies of the last call


def test_stages_builds_filter_then_fill_and_hands_the_reference_on_under_its_keyword():
    calls = []

    def filt(x, *args, **kw):
        calls.append(("filter", x, args, kw))
        return x + 1, kw.get("ref")

    def fill(x, *args, **kw):
        calls.append(("fill", x, args, kw))
        return (x + 10, "filled") if kw.get("ref") is None else (x + 10, "filled", "tallies")

    assert inference._stages(None, None, filt, fill, "ref") == []
    both = inference._stages(dict(min_size=2), dict(connectivity=3), filt, fill, "ref", 16)
    assert inference._run_stages(lambda ref: (0, ref), both, "R") == (11, "tallies")
    assert calls == [("filter", 0, (16,), dict(ref=None, min_size=2)), ("fill", 1, (16,), dict(ref="R", connectivity=3))]
    only_fill = inference._stages(None, dict(), filt, fill, "ref")
    assert inference._run_stages(lambda ref: (0, ref), only_fill, None) == (10, None)
    only_filter = inference._stages(dict(), None, filt, fill, "ref")
    assert inference._run_stages(lambda ref: (0, ref), only_filter, "R") == (1, "R")


@pytest.mark.parametrize("stage,form", list(itertools.product(STAGES, FORMS)))
def test_every_key_of_every_key_tuple_is_accepted(stage, form):
    keys = KEYS[stage, form]
    postprocess.check_stage_kwargs(stage, form, {})
    postprocess.check_stage_kwargs(stage, form, {k: GOOD[k] for k in keys})
    for k in keys:
        postprocess.check_stage_kwargs(stage, form, {k: GOOD[k]})
        postprocess.check_stage_kwargs(stage, form, {k: None} if k in ("cap", "channels", "classes") else {k: GOOD[k]})


@pytest.mark.parametrize("stage,form", list(itertools.product(STAGES, FORMS)))
def test_a_bad_stage_dict_is_refused_with_the_name_of_the_argument(stage, form):
    keys = KEYS[stage, form]

    def refused(value, match):
        with pytest.raises(ValueError, match=match):
            postprocess.check_stage_kwargs(stage, form, value)

    for bad in (dict(size=3), [1], "all", dict(labels=None), dict(reference=None)):      # not a dict, or an unknown key
        refused(bad, stage)
    other = "classes" if form == "mask" else "channels"                                  # the other form's selection key
    refused({other: (1,)}, stage)
    for bad in (0, 4, True, "1", None):
        refused(dict(connectivity=bad), "connectivity")
    for name in ("num_components", "min_size"):
        for bad in (True, 1.5, -1, "2", None):
            if name in keys:
                refused({name: bad}, name)
            else:
                refused({name: 1}, stage)                                                # not a key of this stage at all
    if "cap" in keys:
        for bad in (0, True, 2.0, postprocess.nv.CC_MAX_CAP + 1):
            refused(dict(cap=bad), "cap")
    selection = "channels" if form == "mask" else "classes"
    if (stage, form) != ("postprocess", "mask"):     # those channels go through int() in filter_components, against the mask
        for bad in ("12", b"12", 3, (1.5,), (True,), (-1,)):
            refused({selection: bad}, f"{stage}: {selection}")
    if form == "map":
        refused(dict(classes=(0,)), f"{stage}: classes")
        refused(dict(classes=[2, 0]), f"{stage}: classes")
    elif stage == "fill_holes":
        postprocess.check_stage_kwargs(stage, form, dict(channels=(0,)))                 # channel 0 exists in the mask form


def _never(*args, **kwargs):
    raise AssertionError("the predictor was called")


@pytest.mark.parametrize("bad,match", [(dict(connectivity=4), "connectivity must be 1, 2 or 3, got 4"),
                                       (dict(num_components=True), "num_components must be an integer >= 0, got True"),
                                       (dict(min_size=1.5), "min_size must be an integer >= 0, got 1.5"),
                                       (dict(cap=0), "cap must be an integer in 1..")])
def test_the_mask_form_postprocess_values_are_refused_before_the_predictor_with_filter_components_own_text(bad, match):
    with pytest.raises(ValueError, match=match) as early:
        inference.infer(_never, torch.zeros(1, 1, 8, 8, 8), (8, 8, 8), postprocess=bad)
    with pytest.raises(ValueError) as late:
        postprocess.filter_components(torch.zeros(1, 1, 8, 8, 8), **bad)                 # refused before the device check
    assert str(early.value) == str(late.value)
    # evaluate_volume checks the image's device first, as it always has
    with pytest.raises(RuntimeError, match="MI355X"):
        inference.evaluate_volume(_never, torch.zeros(1, 1, 8, 8, 8), None, (8, 8, 8), postprocess=bad)
