"""The host protocol of the score maps (gc_ens_map_*): what a fresh handle holds, the counters, and the order in which the
five entries report their state faults -- two faults at once at every rung of the ladder, asserting which message wins, the
way tests/test_gpu_host_api.py does it for the other units.  Every refused call ends on the host; nothing is launched."""
import ctypes

import numpy as np
import pytest

from gencast_flax_nnx_amd import _lib
from tests import helpers

pytestmark = pytest.mark.gpu

MAP_COUNTERS = ("ens_map_calls", "ens_map_device_us", "ens_map_invalid_points", "ens_map_blocks", "ens_map_bytes")
FRESH_ALLOCATIONS = 51        # as tests/test_gpu_host_api.py counts them: the buffers of gc_set_graph on the 13 x 24 grid


def test_nothing_is_allocated_before_the_plan_and_the_counters_read_zero():
  nd = helpers.graph_handle(helpers.small_graph(), 1, 2)
  try:
    for name in MAP_COUNTERS:
      assert nd.counter(name) == 0, name
    assert nd.counter("device_allocations") == FRESH_ALLOCATIONS
    for name in ("ens_map", "ens_map_chunks"):
      with pytest.raises(ValueError, match="unknown counter"):
        nd.counter(name)
    G = nd.num_grid_nodes
    nd.ens_map_set([1], 4, 2)
    assert nd.counter("device_allocations") == FRESH_ALLOCATIONS + 5
    assert nd.counter("ens_map_bytes") == 4 * (6 * 8 + 3 * 4 + 2 * 5 * 4) * G
    nd.ens_map_set(None, 1)
    assert nd.counter("device_allocations") == FRESH_ALLOCATIONS + 5
    assert nd.counter("ens_map_bytes") == (6 * 8 + 3 * 4) * G * 2 and nd.counter("ens_map_calls") == 0
  finally:
    nd.close()


def test_the_order_of_the_checks_of_the_map_entries():
  lib = _lib.load_library()
  ST, ARG = _lib.GC_ERR_STATE, _lib.GC_ERR_INVALID_ARGUMENT
  gr = helpers.small_graph()
  G, B, C = gr.num_grid_nodes, 1, 2
  bare = _lib.NativeDenoiser(latent_size=128, d_model=128, num_heads=2, ffw_hidden=256, num_layers=1, c_in=C + 4, c_out=C, batch=B)
  h = helpers.graph_handle(gr, B, C)
  buf = np.zeros(16 * G * B * C)                             # stands for any output: a refused call writes nothing
  D = buf.ctypes.data_as(ctypes.POINTER(ctypes.c_double))
  U = buf.ctypes.data_as(ctypes.POINTER(ctypes.c_uint32))
  field = np.zeros((G, B, C), np.float32)
  F = field.ctypes.data_as(ctypes.POINTER(ctypes.c_float))
  wrong = []

  def expect(what, p, call, code, fragment):
    rc = call(p)
    err = lib.gc_last_error(p).decode()
    print(f"{what}: {rc} {err!r}")
    if rc != code or fragment not in err:
      wrong.append((what, rc, err, code, fragment))

  acc = lambda slot, truth=None: lambda p: lib.gc_ens_map_accumulate(p, slot, truth)
  evs = lambda slot: lambda p: lib.gc_ens_map_accumulate_events(p, slot)
  down = lambda slot, out=True, ev=None: lambda p: lib.gc_ens_map_download(p, slot, D if out else None, U if out else None, ev, None)
  reset = lambda slot: lambda p: lib.gc_ens_map_reset(p, slot)
  GRAPH, PLAN, SLOT, STORE = "gc_set_graph must be called first", "no map plan (gc_ens_map_set)", "slot outside [0, n_slots)", "no member store (gc_ens_reserve)"
  NOT_PUSHED = lambda i: f"member slot {i} has not been pushed"
  TRUTH, MEMBERS = "no truth on the device (pass one to gc_ens_map_accumulate)", "reset the slot first"
  NO_PLANES, OTHER_T, CODES = "the map plan has no event planes", "are not as many as the map plan's", "no event codes on the device"
  try:
    # ---- no graph: it wins over a bad slot, a null output and the missing plan
    p = bare._h
    expect("no graph: set", p, lambda p: lib.gc_ens_map_set(p, 0, None, 0, 99), ST, GRAPH)
    expect("no graph: accumulate", p, acc(99), ST, GRAPH)
    expect("no graph: events", p, evs(99), ST, GRAPH)
    expect("no graph: download", p, down(99, out=False), ST, GRAPH)
    expect("no graph: reset", p, reset(-9), ST, GRAPH)
    # ---- the graph, no plan: the missing plan wins over a bad slot and a null output
    p = h._h
    expect("no plan: accumulate", p, acc(99), ST, PLAN)
    expect("no plan: events", p, evs(99), ST, PLAN)
    expect("no plan: download", p, down(99, out=False), ST, PLAN)
    expect("no plan: reset", p, reset(-9), ST, PLAN)
    # ---- a plan without event planes, no store
    h.ens_map_set(None, 2, 0)
    expect("T = 0: events, bad slot", p, evs(99), ST, NO_PLANES)
    expect("T = 0: download with events", p, down(0, ev=U), ARG, NO_PLANES)
    # ---- a plan with one threshold, no store: the slot wins over the missing store, over a null output
    h.ens_map_set(None, 2, 1)
    expect("no store: accumulate, bad slot", p, acc(2), ARG, SLOT)
    expect("no store: accumulate", p, acc(0), ST, STORE)
    expect("no store: events, bad slot", p, evs(-1), ARG, SLOT)
    expect("no store: events", p, evs(1), ST, STORE)
    expect("no store: download, bad slot and null", p, down(2, out=False), ARG, SLOT)
    expect("no store: download, null", p, down(1, out=False), ARG, "null argument")
    expect("no store: reset, bad slot", p, reset(2), ARG, SLOT)
    # ---- the store reserved, slots unpushed, no truth, no thresholds: the unpushed slot wins over the missing truth;
    # for the events the other T (none set: 0 against 1) wins over the missing codes
    h.ens_reserve(2)
    expect("reserved: accumulate", p, acc(0), ST, NOT_PUSHED(0))
    h.ens_push_host(0, field)
    expect("one unpushed: accumulate", p, acc(0), ST, NOT_PUSHED(1))
    expect("one unpushed: events", p, evs(0), ST, OTHER_T)
    h.ens_push_host(1, field)
    # ---- all pushed, no truth
    expect("all pushed: accumulate, no truth", p, acc(1), ST, TRUTH)
    expect("all pushed: accumulate, no truth, bad slot", p, acc(5), ARG, SLOT)
    # ---- thresholds: two against the plan's one wins over the missing codes; then one, and the codes are missing
    thr = np.zeros((2, G, B, C), np.float32)
    h.ens_event_set(thr, (+1, -1), np.ones(G, np.uint32))
    expect("T = 2 against 1: events", p, evs(0), ST, OTHER_T)
    h.ens_event_set(thr[:1], (+1,), np.ones(G, np.uint32))
    expect("no codes: events", p, evs(0), ST, CODES)
    # ---- a date of M = 2 in slot 0, then a store of M = 3
    assert lib.gc_ens_map_accumulate(p, 0, F) == 0
    assert h.counter("ens_map_calls") == 1 and h.counter("ens_map_invalid_points") == 0
    h.ens_reserve(3)
    expect("M = 3, unpushed: accumulate", p, acc(0), ST, NOT_PUSHED(0))      # the unpushed slot wins over the other M
    for i in range(3):
      h.ens_push_host(i, field)
    expect("M = 3 against 2: accumulate", p, acc(0), ST, MEMBERS)
    expect("M = 3 against 2: accumulate with a truth", p, acc(0, F), ST, MEMBERS)
    expect("M = 3 against 2: events, no codes", p, evs(0), ST, CODES)         # the missing codes win over the other M
    h.ens_event_score(field)
    expect("M = 3 against 2: events", p, evs(0), ST, MEMBERS)
    # the other slot takes the new M; a reset lets slot 0 take it too
    assert lib.gc_ens_map_accumulate(p, 1, None) == 0 and lib.gc_ens_map_accumulate_events(p, 1) == 0
    assert lib.gc_ens_map_reset(p, 0) == 0
    assert lib.gc_ens_map_accumulate_events(p, 0) == 0 and lib.gc_ens_map_accumulate(p, 0, None) == 0
    dates = np.zeros(2, np.int64)
    assert lib.gc_ens_map_download(p, 0, D, U, None, dates.ctypes.data_as(ctypes.POINTER(ctypes.c_int64))) == 0
    assert dates.tolist() == [1, 1] and h.counter("ens_map_calls") == 5
    # the codes go with the store
    h.ens_reserve(3)
    for i in range(3):
      h.ens_push_host(i, field)
    expect("after a reserve: events", p, evs(0), ST, CODES)
    assert not wrong, "\n".join(f"{w[0]}: got {w[1]} {w[2]!r}, expected {w[3]} with {w[4]!r}" for w in wrong)
  finally:
    h.close()
    bare.close()
