"""csrc/graph_cache.h when arguments move, vanish or thrash.

Every training-mode call of the decoder stack, the frozen-BatchNorm stack backward and the PointNet encoder is keyed by what
its `fill` lambda adds; from the third call with a key on it is ONE hipGraphLaunch that holds ADDRESSES.  The rest of the
suite drives the cache with the same pointers step after step, the one situation in which a key that misses an argument
cannot show.  Here one argument at a time moves, changes, vanishes or comes back, for all six entries.

Reference of every check: the same entry with the same arguments with recording switched off
(dpf_train_graph_set_enabled(0)), bit for bit.  No tolerance anywhere: the kernels are deterministic, and other tests anchor
the eager path to float64 and to the goldens.

Counters: deltas of dpf_train_graph_stats = (replays, eager, records, evictions, uncapturable), process-wide, so these tests
are single-threaded.  From GraphCache::run: a key seen for the first time runs eagerly (eager +1; evictions +1 if and only if
all eight slots of the entry's cache were taken -- which depends on what ran earlier in the process, hence 0 or 1 here
except where the test itself has filled the slots); the second call records AND launches the recording (records +1,
replays +1); every later call is replays +1.  Three calls with a fresh key: FRESH = replays 2, eager 1, records 1.

Safety: every buffer any call has used stays alive until the process ends (graph_cases.ALIVE), so a replay through a stale
key lands in live memory and the test fails by comparison, never by a fault.  Every library call is followed by
torch.cuda.synchronize() before anything is compared and before the next call, because the next call may evict and destroy
an executable graph: whether the runtime tolerates the destruction of an executable that is still in flight is NOT examined
here.  Neither is a second thread."""
import ctypes

import pytest
import torch

from tests import graph_cases as GC

pytestmark = pytest.mark.gpu

FRESH = (2, 1, 1, 0)           # replays, eager, records, uncapturable of three calls with a key never seen before
REPLAYS3 = (3, 0, 0, 0)        # ... of three calls with a key that is a graph already


def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")


class recording:
    """recording switched on (or off) for a test, the previous state (DPF_TRAIN_GRAPH=0 in the environment) restored after it"""

    def __init__(self, on=1):
        self.on = on

    def __enter__(self):
        self.prev = GC.set_enabled(self.on)

    def __exit__(self, *exc):
        GC.set_enabled(self.prev)


def _delta(s0):
    return tuple(a - b for a, b in zip(GC.stats(), s0))


def _same(got, ref, what):
    assert set(got) == set(ref), (what, sorted(got), sorted(ref))
    for k in ref:
        assert torch.equal(got[k], ref[k]), "%s: `%s` differs from the recording-off result" % (what, k)


def _differs(a, b):
    return any(not torch.equal(a[k], b[k]) for k in a if k in b)


def _calls(call, ref, expect, what, n=3, after=None):
    """n calls of `call`: each returns the reference's code and leaves the reference's outputs; the counters move by `expect`"""
    rc0, out0 = ref
    s0 = GC.stats()
    for i in range(n):
        assert call.invoke() == rc0, (what, i)
        _same(call.outputs(), out0, "%s, call %d" % (what, i))
        if after is not None:
            after("%s, call %d" % (what, i))
    d = _delta(s0)
    assert (d[0], d[1], d[2], d[4]) == expect, (what, d)
    assert 0 <= d[3] <= expect[1], (what, d)                     # only a first sighting can evict


def _established(entry, seed=1, **over):
    """a fresh argument set, its reference, three calls: the key is a graph"""
    call = GC.build(entry, seed, **over)
    ref = GC.reference(call)
    assert ref[0] == 0, (entry, ref[0])
    _calls(call, ref, FRESH, "%s base" % entry)
    return call, ref


# ---- 1. one pointer moves ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("entry,name", GC.DEVICE_POINTERS)
def test_one_pointer_moves(entry, name):
    """The base set is a graph.  Then ONE device pointer is another buffer: an input with other contents, an output (and the
    buffer it replaces) full of canary.  Three calls: a fresh key, the recording-off result of exactly these arguments each
    time, and the replaced buffer untouched."""
    _gpu()
    with recording():
        a, ref_a = _established(entry)
        b = GC.build(entry, 2)
        role, old = GC.role(entry, name), a.values[name]
        if (entry, name) == ("dpf_encoder_train_backward", "pooled"):
            # the backward reads only whether a pooled feature is positive (all are, in both sets): in the other set every second
            # feature is dead, a pooled value of exactly zero
            b.values[name].t[:, ::2] = 0
        a2 = a.with_values(**{name: b.values[name]})
        ref2 = GC.reference(a2)
        assert ref2[0] == 0
        written = role in (GC.OUT, GC.INOUT, GC.SCRATCH)
        if written:
            GC.fill_canary(old.t)
        elif name == "meta_dev":
            # the table on the device has to agree with meta_host, so its copy cannot differ: the OLD one changes instead (rows
            # rotated, still a valid table), and a replay that still reads it is seen
            old.t.copy_(old.t.roll(1, 0))
            assert _differs(GC.reference(a)[1], ref2[1])
        else:
            assert _differs(ref_a[1], ref2[1]), "the outputs do not depend on `%s`: the case cannot see a stale pointer" % name

        def holds(what):
            assert GC.holds_canary(old.t), "%s: the replaced `%s` was written" % (what, name)
        _calls(a2, ref2, FRESH, "%s with another `%s`" % (entry, name), after=holds if written else None)


# ---- 2. one scalar changes, pointers unchanged ---------------------------------------------------------------------------
@pytest.mark.parametrize("entry,name", [(e, n) for e, n in GC.SCALARS if (e, n) not in GC.NO_SECOND_VALUE])
def test_one_scalar_changes(entry, name):
    """The base set is a graph.  The same buffers, holding the (smaller) call's data, with ONE scalar at its second value: a
    fresh key and the recording-off results.  Back at the first value the next call is a replay at once."""
    _gpu()
    with recording():
        a, ref_a = _established(entry)
        second = GC.second_value(entry, name, a.kwargs)
        v = GC.build(entry, 1, **second)                         # that call's own consistent state ...
        assert v.values[name] != a.values[name]
        changed = [n for n, r, _ in a.roles() if r == GC.SCALAR and v.values[n] != a.values[n]]
        assert changed == [name], changed
        keep = a.contents()
        a.load(v)                                                # ... in the front of the base call's buffers
        a2 = a.with_values(**{name: v.values[name]})
        ref2 = GC.reference(a2)
        assert ref2[0] == 0
        _calls(a2, ref2, FRESH, "%s with %s = %r" % (entry, name, v.values[name]))
        GC.restore(keep)
        _calls(a, ref_a, (1, 0, 0, 0), "%s back at the first %s" % (entry, name), n=1)


# ---- 3. the host tables --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("entry", GC.STACK_ENTRIES)
def test_meta_host_is_keyed_by_content(entry):
    """The rows of layers 0 and 1 of the same ctypes array change places (warp [0] / [1] of a pattern-0 triple: two kept
    coordinates and one warped each, so their parameter blocks have the same shape): another valid table at the same address."""
    _gpu()
    with recording():
        a, ref_a = _established(entry)
        t = a.values["meta_host"]
        rows = list(t.items)
        assert sorted(rows[0:2]) != sorted(rows[4:6]) and (rows[1] >= 0) == (rows[5] >= 0) and (rows[3] >= 0) == (rows[7] >= 0)
        for i in range(4):
            t.set(i, rows[4 + i])
            t.set(4 + i, rows[i])
        ref2 = GC.reference(a)
        assert ref2[0] == 0 and _differs(ref_a[1], ref2[1])
        _calls(a, ref2, FRESH, "%s with the meta rows exchanged in place" % entry)


@pytest.mark.parametrize("entry,name", [(e, n) for e, n in GC.HOST_TABLES if n != "meta_host"])
def test_pointer_tables_are_keyed_by_content(entry, name):
    """The per-layer gradient tables and the encoder's `running`: the same contents at a new host address hit; one entry
    changed in place, one entry NULL, and the whole table NULL each miss."""
    _gpu()
    running = name == "running"
    with recording():
        a, ref_a = _established(entry)
        b = GC.build(entry, 2)
        t = a.values[name]
        # the same contents at another host address: a replay
        moved = a.with_values(**{name: t.rebuilt()})
        assert ctypes_address(moved.values[name]) != ctypes_address(t)
        _calls(moved, ref_a, (1, 0, 0, 0), "%s, `%s` rebuilt elsewhere" % (entry, name), n=1)
        # one entry changed in place
        # running: the mean of layer 1 (et_bn_finish_kernel guards BOTH updates of a layer by the mean's pointer: only a mean
        # entry may be NULL, and then neither statistic of that layer moves)
        i = 2 if running else 1
        was = t.items[i]
        t.set(i, b.values[name].items[i])
        if running:
            was.t.copy_(was.snap)                                # no call restores it any more; none may move it either
        ref2 = GC.reference(a)
        assert ref2[0] == 0 and _differs(ref_a[1], ref2[1])

        def untouched(what):
            assert torch.equal(was.t, was.snap), "%s: the replaced running statistic moved" % what

        def idle(what):
            for j, item in enumerate(t.items):
                assert item is None or torch.equal(item.t, item.snap), "%s: running[%d] moved without `running`" % (what, j)
            untouched(what)
        _calls(a, ref2, FRESH, "%s, %s[%d] changed in place" % (entry, name, i), after=untouched if running else None)
        # one entry NULL
        t.set(i, None)
        ref3 = GC.reference(a)
        assert ref3[0] == 0 and _differs(ref2[1], ref3[1])
        _calls(a, ref3, FRESH, "%s, %s[%d] NULL" % (entry, name, i), after=untouched if running else None)
        if not running:                                          # ... which is the result of a zero gradient
            t.set(i, GC.Buf(torch.zeros_like(was.t)))
            zero = GC.reference(a)[1]
            for k in zero:
                assert torch.equal(zero[k].view(torch.float32), ref3[1][k].view(torch.float32)), (entry, name, k)
            t.set(i, None)
        # the whole table NULL after it was present
        gone = a.with_values(**{name: None})
        ref4 = GC.reference(gone)
        assert ref4[0] == 0
        if running:
            for item in t.items:
                if item is not None:
                    item.t.copy_(item.snap)
        _calls(gone, ref4, FRESH, "%s without `%s`" % (entry, name), after=idle if running else None)


def ctypes_address(table):
    return ctypes.addressof(table.c)


# ---- 4. optional arguments appear and vanish -----------------------------------------------------------------------------
@pytest.mark.parametrize("entry,name", [("dpf_flow_train_backward", "g_mus"), ("dpf_flow_train_backward", "g_lvs"),
                                        ("dpf_encoder_train_backward", "dx"), ("dpf_encoder_train_forward", "batch_stats"),
                                        ("dpf_encoder_train_forward", "running")])
def test_optional_argument_vanishes_and_returns(entry, name):
    """present -> NULL -> present with everything else fixed, three calls each.  In the NULL phase the buffer that used to be
    passed keeps its canary (`running`: the statistics do not move); the third phase replays at once."""
    _gpu()
    with recording():
        a, ref_a = _established(entry)
        was = a.values[name]
        none = a.with_values(**{name: None})
        ref0 = GC.reference(none)
        assert ref0[0] == 0
        if GC.role(entry, name) == GC.IN:
            assert _differs({k: v for k, v in ref_a[1].items()}, ref0[1])
            after = None
        elif name == "running":
            for item in was.items:
                item.t.copy_(item.snap)

            def after(what):
                for j, item in enumerate(was.items):
                    assert torch.equal(item.t, item.snap), "%s: running[%d] moved" % (what, j)
        else:
            GC.fill_canary(was.t)

            def after(what):
                assert GC.holds_canary(was.t), "%s: `%s` was written" % (what, name)
        _calls(none, ref0, FRESH, "%s without `%s`" % (entry, name), after=after)
        _calls(a, ref_a, REPLAYS3, "%s with `%s` again" % (entry, name))


# ---- 5. two live sets, then nine -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("entry", ["dpf_flow_train_backward_lists", "dpf_encoder_train_forward"])
def test_two_live_sets_then_nine(entry):
    """Two sets that differ in every buffer, in turn: from the third round on every call is a replay of its own graph.  Nine
    sets in turn, one more than SLOTS: every call is a first sighting that evicts the least recently used key -- the next one
    to be called -- so `evictions` grows with every call from the ninth on and `replays` stands still (graph_cache.h)."""
    _gpu()
    with recording():
        sets = [GC.build(entry, s) for s in (1, 2)]
        refs = [GC.reference(c) for c in sets]
        assert _differs(refs[0][1], refs[1][1])
        for rnd in range(6):
            for c, ref in zip(sets, refs):
                s0 = GC.stats()
                assert c.invoke() == ref[0] == 0
                _same(c.outputs(), ref[1], "%s, two sets, round %d" % (entry, rnd))
                d = _delta(s0)
                want = [(0, 1, 0, 0), (1, 0, 1, 0)][rnd] if rnd < 2 else (1, 0, 0, 0)
                assert (d[0], d[1], d[2], d[4]) == want and d[3] <= want[1], (entry, rnd, d)
        sets = [GC.build(entry, 10 + s) for s in range(9)]
        refs = [GC.reference(c) for c in sets]
        n = 0
        for rnd in range(3):
            for c, ref in zip(sets, refs):
                s0 = GC.stats()
                assert c.invoke() == ref[0] == 0
                _same(c.outputs(), ref[1], "%s, nine sets, round %d" % (entry, rnd))
                d = _delta(s0)
                assert (d[0], d[1], d[2], d[4]) == (0, 1, 0, 0), (entry, rnd, n, d)
                assert d[3] == 1 if n >= 8 else d[3] in (0, 1), (entry, rnd, n, d)     # our own eight keys fill the slots
                n += 1


# ---- 6. calls that cannot be recorded ------------------------------------------------------------------------------------
@pytest.mark.parametrize("entry,name", [("dpf_flow_train_forward", "B"), ("dpf_encoder_train_forward", "N"),
                                        ("dpf_encoder_train_backward", "N")])
def test_rejected_call_is_uncapturable_and_leaves_nothing_behind(entry, name):
    """A size of zero is refused inside `direct`, behind the cache: first sighting eager, the recording fails (uncapturable +1)
    and falls back to the direct call, the third call finds the key marked and goes direct: eager +3, nothing recorded,
    nothing replayed, the same code each time, no output written.  The entry then serves a valid call as any fresh key."""
    _gpu()
    with recording():
        a = GC.build(entry, 1)
        bad = a.with_values(**{name: 0})
        s0 = GC.stats()
        codes = []
        for i in range(3):
            codes.append(bad.invoke())
            for n, r, b in bad.bufs():
                if r in (GC.OUT, GC.SCRATCH):
                    assert GC.holds_canary(b.t), (entry, i, n)
                elif b.snap is not None:
                    assert torch.equal(b.t, b.snap), (entry, i, n)
        assert codes == [-1, -1, -1], codes
        d = _delta(s0)
        assert (d[0], d[1], d[2], d[4]) == (0, 3, 0, 1) and d[3] <= 1, d
        _calls(a, GC.reference(a), FRESH, "%s, a valid call afterwards" % entry)


# ---- 7. switched off and on again ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("entry", ["dpf_flow_train_forward", "dpf_flow_frozen_backward_lists", "dpf_encoder_train_backward"])
def test_switched_off_and_on_again(entry):
    _gpu()
    with recording():
        a, ref = _established(entry)
        assert GC.set_enabled(0) == 1
        try:
            s0 = GC.stats()
            for i in range(2):
                assert a.invoke() == 0
                _same(a.outputs(), ref[1], "%s, recording off, call %d" % (entry, i))
            assert _delta(s0) == (0, 0, 0, 0, 0)
        finally:
            assert GC.set_enabled(1) == 0
        _calls(a, ref, (1, 0, 0, 0), "%s, recording on again" % entry, n=1)


# ---- 8. inside the caller's own capture ----------------------------------------------------------------------------------
@pytest.mark.parametrize("entry,moving", [("dpf_flow_train_backward_lists", "g_ps[0]"), ("dpf_encoder_train_forward", "x")])
def test_call_inside_the_callers_capture_passes_through(entry, moving):
    """One eager call first (the one-time per-device setup).  The same call inside torch.cuda.graph on a side stream goes into
    the CALLER's capture: the library records nothing of its own and no counter moves.  The torch graph, replayed on changed
    input contents, gives the recording-off result for those contents."""
    _gpu()
    with recording():
        a = GC.build(entry, 1)
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            a.reset()
            assert a.launch() == 0
        torch.cuda.synchronize()
        s0 = GC.stats()
        a.reset()
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.stream(side):
            with torch.cuda.graph(graph, stream=side):
                rc = a.launch()
        torch.cuda.synchronize()
        assert rc == 0 and _delta(s0) == (0, 0, 0, 0, 0), (rc, _delta(s0))
        buf = dict((n, b) for n, _, b in a.bufs())[moving]
        last = None
        for it in range(2):
            buf.t.mul_(1.25).add_(0.125 * (it + 1))
            ref = GC.reference(a)
            assert ref[0] == 0 and (last is None or _differs(last, ref[1]))
            last = ref[1]
            a.reset()
            torch.cuda.synchronize()
            graph.replay()
            torch.cuda.synchronize()
            _same(a.outputs(), ref[1], "%s, the caller's graph, replay %d" % (entry, it))
        assert _delta(s0) == (0, 0, 0, 0, 0)
        GC.ALIVE.append(graph)


# ---- 9. through the modules ----------------------------------------------------------------------------------------------
def _decoder_run(nets, seed, steps=6):
    from oracle import flow_oracle as FO
    torch.manual_seed(seed)
    dec = nets.LocalCondRNVPDecoder(1, 64, 64).cuda().train()
    store = dec.flatten_parameters()
    opt = nets.Adam(list(dec.parameters()), lr=1e-3, weight_decay=1e-6, betas=(0.9, 0.999), amsgrad=True)
    tgt, _, g = FO.synthetic_inputs(seed, 4, 33, 64)
    n = store.flat_p.numel()
    # the trajectory goes into storage allocated up front: a step that kept a new tensor would never see the allocator settle,
    # and no call would ever be a replay
    traj = {"loss": torch.zeros(steps, device="cuda"), "gradient": torch.zeros((steps, n), device="cuda"),
            "weights": torch.zeros((steps, n), device="cuda")}
    run = {"dec": dec, "store": store, "opt": opt, "tp": torch.from_numpy(tgt).cuda(), "tg": torch.from_numpy(g).cuda(), "traj": traj,
           "step": 0}
    GC.ALIVE.append(run)
    return run


def _decoder_step(run):
    i, traj = run["step"], run["traj"]
    run["opt"].zero_grad(set_to_none=True)
    ps, mus, lvs = run["dec"](run["tp"], run["tg"], mode="inverse")
    loss = ps[0].square().mean() + sum(lvs).mean()
    loss.backward()
    traj["loss"][i].copy_(loss.detach())
    traj["gradient"][i].copy_(run["store"].flat_g.detach())
    run["opt"].step()
    traj["weights"][i].copy_(run["store"].flat_p.detach())
    torch.cuda.synchronize()
    run["step"] = i + 1


def test_alternating_decoders_follow_their_own_trajectories():
    """Two decoders of the same shape train in turn, six optimizer steps each, in one process: two live pointer sets per entry.
    Each follows, bit for bit (loss, gradient and weights of every step), the trajectory it has when trained alone with
    recording off.  Some of the calls must have been replays, or the run has shown nothing."""
    _gpu()
    from dpf_nets_amd import networks as nets
    alone = []
    with recording(0):
        for seed in (1, 2):
            run = _decoder_run(nets, seed)
            for _ in range(6):
                _decoder_step(run)
            alone.append(run["traj"])
    with recording():
        runs = [_decoder_run(nets, seed) for seed in (1, 2)]
        s0 = GC.stats()
        for _ in range(6):
            for run in runs:
                _decoder_step(run)
        d = _delta(s0)
    print("alternating decoders: counters moved by", d)
    assert d[0] + d[1] == 24 and d[4] == 0, d                    # 2 decoders x 6 steps x (forward + backward), each eager or a graph
    assert d[0] >= 1, d
    for seed, run, ref in zip((1, 2), runs, alone):
        for what in ("loss", "gradient", "weights"):
            for i in range(6):
                assert torch.equal(run["traj"][what][i], ref[what][i]), "decoder %d leaves its own trajectory at step %d (%s)" % (seed, i, what)


def _short_batch_run(nets, on):
    batches = (4, 4, 4, 3, 4, 4)
    with recording(on):
        torch.manual_seed(7)
        enc = nets.PointNetCloudEncoder(3, 64, [128, 256, 512]).cuda().train()
        dec = nets.LocalCondRNVPDecoder(1, 64, 512).cuda().train()
        gen = torch.Generator(device="cuda").manual_seed(7)
        x_all = torch.randn((4, 3, 33), device="cuda", generator=gen)
        params = list(enc.parameters()) + list(dec.parameters())
        # (storage allocated up front, as in _decoder_run)
        losses = torch.zeros(len(batches), device="cuda")
        grads = [[torch.zeros_like(p) for p in params] for _ in batches]
        GC.ALIVE.append((enc, dec, x_all, losses, grads))
        s0 = GC.stats()
        for i, b in enumerate(batches):
            for p in params:
                if p.grad is not None:
                    p.grad.zero_()                               # in place: the gradients keep their addresses
            x = x_all[:b]
            g = torch.max(enc(x), dim=2)[0]
            ps, mus, lvs = dec(x, g, mode="inverse")
            loss = ps[0].square().mean() + sum(lvs).mean()
            loss.backward()
            assert all(p.grad is not None for p in params)
            losses[i].copy_(loss.detach())
            with torch.no_grad():
                torch._foreach_copy_(grads[i], [p.grad for p in params])
                for p in params:
                    p.add_(p.grad, alpha=-1e-3)
            torch.cuda.synchronize()
            del g, ps, mus, lvs, loss                            # or the steps alternate between two sets of blocks and none replays
        return [[losses[i]] + grads[i] for i in range(len(batches))], _delta(s0)


def test_a_short_last_batch_through_encoder_and_decoder():
    """One PointNetCloudEncoder and one decoder in train() are stepped with batch sizes 4, 4, 4, 3, 4, 4 (the short batch is a
    new key between steps that may replay): every loss and every gradient equals those of the recording-off run."""
    _gpu()
    from dpf_nets_amd import networks as nets
    ref, d0 = _short_batch_run(nets, 0)
    got, d1 = _short_batch_run(nets, 1)
    print("short last batch: counters moved by", d1)
    assert d0 == (0, 0, 0, 0, 0)
    assert d1[0] + d1[1] == 24 and d1[4] == 0, d1                # 6 steps x 4 cached calls, each eager or a graph
    assert d1[0] >= 1, d1                                        # some were replays, or the run has shown nothing
    for step, (a, b) in enumerate(zip(got, ref)):
        assert len(a) == len(b)
        for i, (x, y) in enumerate(zip(a, b)):
            assert torch.equal(x, y), "step %d: %s differs from the recording-off run" % (step, "the loss" if i == 0 else "gradient %d" % (i - 1))
