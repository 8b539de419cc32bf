"""The counting build's diagnostics (cr_get_diag, DIAG_* in csrc/kernels.hpp): the leaf-round census and
the repeated-miss census that the trace kernels keep beside the traversal (csrc/travprobe.hpp).

Each case is one counting render (option counters 1) with diag_kinds 7 (camera, closest and shadow traces)
and every generation in its own wf_trace launches -- wf_tail passes no Diag, so a tail launch would leave
its rounds and tests out of the census.  (That is option wf_tail_min 0, "never hand a queue to wf_tail":
a queue SHORTER than wf_tail_min goes to the tail, so a large value would send everything there; the case
asserts that no tail launch ran.)  The relations are read off the code:

  tests    == the three traces' tritest counters (both count every test that passes the exclude check)
  geomiss  <= tests, rep1 <= rep4 <= rep8 <= geomiss (a window of 1 / 4 / 8 last misses)
  rounds, distinct, records == counters leaf_rounds, leaf_distinct, leaf_records (the same block, same leader)
  fit64 <= fit128 <= rounds, distinct <= lanes <= 64 * rounds, records <= lanetests
  rounds + urounds == counters wave_round (every leaf round is divergent or uniform)
  diag_kinds 0: every slot 0

All of them hold on the code before the census moved into the probe; none had to be dropped.

The per-lane sums (tests, geomiss, rep1, rep4, rep8) follow a ray through its own query only, so they do
not depend on which wave took which ray: two renders gave the same values, and tests/golden/diag_parent.json
holds them as recorded before the move.  The round-shape slots depend on the refill order and are not pinned.
"""
import json
import os

import pytest

from helpers import Pair

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "diag_parent.json")
LANE_SUMS = ("tests", "geomiss", "rep1", "rep4", "rep8")
# scene, xres, yres, samples, depth
SHAPES = {"cornell": (16, 16, 2, 6), "sponza": (96, 54, 3, 6)}


@pytest.fixture(scope="module")
def pairs(ca, po, scenes):
    return {name: Pair(ca, po, scenes.config_rtc(name)) for name in SHAPES}


def render_diag(ca, pair, shape, kinds):
    """(diag, counters, trace_stats) of one counting render with diag_kinds = kinds."""
    x, y, s, k = shape
    dev = pair.dev
    dev.set_option("kernel", 2)
    dev.set_option("counters", 1)
    dev.set_option("wf_tail_min", 0)
    dev.set_option("diag_kinds", kinds)
    try:
        dev.render(pair.camera(ca, x, y), ca.render_params(x, y, s, k, 0xC41A05C0, layer=1), None)
        return dev.diag(), dev.counters(), dev.trace_stats()
    finally:  # (kernel 2, counters 1 and wf_tail_min 0 are what Pair and the neighbouring tests leave set)
        dev.set_option("diag_kinds", 0)


@pytest.mark.parametrize("name", list(SHAPES))
def test_diag_census_consistent_with_counters(ca, pairs, name):
    d, c, ts = render_diag(ca, pairs[name], SHAPES[name], 7)
    print(name, d, {k: c[k] for k in ("leaf_rounds", "leaf_distinct", "leaf_records", "wave_round")})
    assert pairs[name].dev.last_trace_build() == -1 and ts["tail"]["launches"] == 0, ts
    assert d["tests"] == sum(ts[k]["tritest"] for k in ("camera", "closest", "shadow")) > 0
    assert d["geomiss"] <= d["tests"]
    assert d["rep1"] <= d["rep4"] <= d["rep8"] <= d["geomiss"]
    assert (d["rounds"], d["distinct"], d["records"]) == (c["leaf_rounds"], c["leaf_distinct"], c["leaf_records"])
    assert d["fit64"] <= d["fit128"] <= d["rounds"]
    assert d["distinct"] <= d["lanes"] <= 64 * d["rounds"]
    assert d["records"] <= d["lanetests"]
    assert d["rounds"] + d["urounds"] == c["wave_round"] > 0
    if name == "sponza":
        assert d["rounds"] > 0 and d["maxcount"] > 0  # the shape that is here for its divergent leaf rounds
    # the lane sums: the same in a second render, and as recorded before the census moved
    d2 = render_diag(ca, pairs[name], SHAPES[name], 7)[0]
    assert {k: d2[k] for k in LANE_SUMS} == {k: d[k] for k in LANE_SUMS}
    with open(GOLDEN) as f:
        assert {k: d[k] for k in LANE_SUMS} == json.load(f)[name]


@pytest.mark.parametrize("name", list(SHAPES))
def test_diag_off_leaves_every_slot_zero(ca, pairs, name):
    d, c, _ = render_diag(ca, pairs[name], SHAPES[name], 0)
    assert all(v == 0 for v in d.values()), d
    assert c["wave_round"] > 0
