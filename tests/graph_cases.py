"""Argument sets of the six graph-cached training entries (csrc/graph_cache.h), for tests/test_gpu_graph_cache.py and
tests/test_graph_cache_cpu.py.  Importable without a GPU: torch and the library are imported inside the builders.

ENTRIES lists, per entry, the source file of its `fill` lambda and every parameter of its C signature but `stream`, in
order, with a role:

  scalar   passed by value
  host     a host array, keyed by CONTENT (meta_host: ints; the gradient tables and `running`: device pointers)
  in       a device buffer the entry only reads
  out      a device buffer the entry only writes (filled with the canary before every call, compared afterwards)
  inout    a device buffer the entry reads and writes (restored from its snapshot before every call, compared afterwards)
  scratch  a device buffer the entry writes whose contents mean nothing afterwards (canary before every call, not compared)

A `Call` is one entry with one value per parameter.  Calls made from the same `Buf` objects share device memory, which is how
the tests swap ONE argument between two calls.  Every built state is kept alive until the process ends (ALIVE): a test that
finds a hole in a key makes a recorded graph touch a buffer of an earlier call, which then is live memory, and addresses are
never handed out twice, so a key is fresh when a test says it is."""
import ctypes
import os

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "dpf_nets_amd", "csrc")

SCALAR, HOST, IN, OUT, INOUT, SCRATCH = "scalar", "host", "in", "out", "inout", "scratch"

_STACK_HEAD = (("n_layers", SCALAR), ("B", SCALAR), ("N", SCALAR), ("mode", SCALAR), ("precision", SCALAR), ("meta_host", HOST))
_STACK_SAVED = (("p_in", IN), ("ps", IN), ("mus", IN), ("logvars", IN))
_STACK_TAIL = (("dp_in", OUT), ("dp_tmp", SCRATCH), ("dcanon", OUT), ("dfm", OUT), ("flow_eps", SCALAR), ("workspace", SCRATCH))
_TRAIN_SAVED = (("tcanon", IN), ("packed", IN), ("film", IN), ("stats", IN)) + _STACK_SAVED

ENTRIES = {
    "dpf_flow_train_forward": ("flow_train.hip", _STACK_HEAD + (
        ("meta_dev", IN), ("tcanon", IN), ("packed", INOUT), ("fm", IN), ("p_in", IN), ("ps", OUT), ("mus", OUT), ("logvars", OUT),
        ("stats", OUT), ("film", OUT), ("flow_eps", SCALAR), ("workspace", SCRATCH))),
    "dpf_flow_train_backward": ("flow_train.hip", _STACK_HEAD + _TRAIN_SAVED + (
        ("g_ps", IN), ("g_mus", IN), ("g_lvs", IN)) + _STACK_TAIL),
    "dpf_flow_train_backward_lists": ("flow_train.hip", _STACK_HEAD + _TRAIN_SAVED + (
        ("g_ps", HOST), ("g_mus", HOST), ("g_lvs", HOST)) + _STACK_TAIL),
    "dpf_flow_frozen_backward_lists": ("flow_frozen.hip", _STACK_HEAD + (
        ("tcanon", IN), ("fstats", IN), ("packed", IN), ("film", IN), ("fm", IN)) + _STACK_SAVED + (
        ("g_ps", HOST), ("g_mus", HOST), ("g_lvs", HOST)) + _STACK_TAIL),
    "dpf_encoder_train_forward": ("encoder_train.hip", (
        ("B", SCALAR), ("N", SCALAR), ("precision", SCALAR), ("canon", IN), ("x", IN), ("ws", OUT), ("pooled", OUT),
        ("batch_stats", OUT), ("running", HOST), ("momentum", SCALAR))),
    "dpf_encoder_train_backward": ("encoder_train.hip", (
        ("B", SCALAR), ("N", SCALAR), ("canon", IN), ("x", IN), ("ws", INOUT), ("pooled", IN), ("g_pooled", IN), ("dcanon", OUT),
        ("dx", OUT))),
}
STACK_ENTRIES = tuple(e for e in ENTRIES if e.startswith("dpf_flow_"))
ENCODER_ENTRIES = tuple(e for e in ENTRIES if e.startswith("dpf_encoder_"))
# (entry, argument name, role), every parameter of every entry
ARGUMENTS = [(entry, name, role) for entry, (_, args) in ENTRIES.items() for name, role in args]
DEVICE_POINTERS = [(e, n) for e, n, r in ARGUMENTS if r in (IN, OUT, INOUT, SCRATCH)]
HOST_TABLES = [(e, n) for e, n, r in ARGUMENTS if r == HOST]
SCALARS = [(e, n) for e, n, r in ARGUMENTS if r == SCALAR]

# the base call of an entry (builder keywords), and the second value each scalar takes with the pointers unchanged: every
# buffer of the base call is large enough for it
BASE = {"stack": dict(n_layers=3, B=2, N=33, mode="inverse", precision="bf16x6", flow_eps=None),
        "frozen": dict(n_layers=3, B=2, N=33, mode="inverse", precision="f16x3", flow_eps=None),
        "encoder": dict(B=2, N=33, precision="bf16x3", momentum=0.1)}
NO_SECOND_VALUE = {("dpf_flow_frozen_backward_lists", "precision"): "the frozen backward accepts f16x3 only"}


def family(entry):
    return "encoder" if entry in ENCODER_ENTRIES else "frozen" if "frozen" in entry else "stack"


def second_value(entry, name, kwargs):
    """builder keywords of the call whose scalar `name` has its second value; None = the entry has no second value for it"""
    if (entry, name) in NO_SECOND_VALUE:
        return None
    v = kwargs.get(name)
    if name == "n_layers":
        return dict(n_layers=2)
    if name == "B":
        return dict(B=1)
    if name == "N":
        return dict(N=31)
    if name == "mode":
        return dict(mode="direct" if v == "inverse" else "inverse")
    if name == "precision":
        return dict(precision={"bf16x6": "bf16x3", "bf16x3": "bf16x6"}[v])
    if name == "flow_eps":
        return dict(flow_eps="double")           # twice the layers' own eps
    if name == "momentum":
        return dict(momentum=0.25)
    raise KeyError((entry, name))


def role(entry, name):
    return dict(ENTRIES[entry][1])[name]


# ---- reading the C sources (no GPU) --------------------------------------------------------------------------------------
def signature_and_fill(entry):
    """([parameter names of the C signature], text of the entry's fill lambda), read from the .hip source"""
    import re
    src = open(os.path.join(CSRC, ENTRIES[entry][0])).read()
    m = re.search(r'extern "C" int %s\((.*?)\)\s*\{' % re.escape(entry), src, re.S)
    assert m, "no definition of %s in %s" % (entry, ENTRIES[entry][0])
    params = [re.findall(r"\w+", p)[-1] for p in m.group(1).split(",")]
    body = src[m.end():]
    body = body[:body.index("\n}\n")]                            # the entry's own body
    call = body.index("dpf_graph_call(")
    fill = body[body.index("[&](GraphKey &k)", call):]
    return params, fill


# ---- values of a call ----------------------------------------------------------------------------------------------------
CANARY = 0xA5
ALIVE = []


class Buf:
    """a device tensor as an argument; snap: what reset() restores it to (inout buffers, running statistics)"""

    def __init__(self, t, snap=None):
        assert t.is_contiguous()
        self.t, self.snap = t, snap

    def bytes(self):
        import torch
        return self.t.view(torch.uint8).reshape(-1)


def inout(t):
    return Buf(t, t.clone())


class Table:
    """a host array: kind "int" (items: ints) or "ptr" (items: Buf or None); .c is the ctypes array the entry reads"""

    def __init__(self, kind, items):
        self.kind, self.items = kind, list(items)
        ctype = ctypes.c_int if kind == "int" else ctypes.c_void_p
        self.c = (ctype * len(self.items))()
        for i in range(len(self.items)):
            self.set(i, self.items[i])

    def set(self, i, item):                                      # IN PLACE: the array keeps its address
        self.items[i] = item
        self.c[i] = item if self.kind == "int" else (None if item is None else item.t.data_ptr())

    def rebuilt(self):                                           # the same contents at a new host address
        return Table(self.kind, self.items)


def fill_canary(t):
    import torch
    t.view(torch.uint8).fill_(CANARY)


def holds_canary(t):
    import torch
    return bool((t.view(torch.uint8) == CANARY).all())


class Call:
    def __init__(self, entry, values, kwargs=None, keep=None):
        names = [n for n, _ in ENTRIES[entry][1]]
        assert list(values) == names, (entry, list(values), names)
        self.entry, self.values, self.kwargs, self.keep = entry, dict(values), dict(kwargs or {}), keep

    def with_values(self, **changes):
        assert all(k in self.values for k in changes), changes
        v = dict(self.values)
        v.update(changes)
        c = Call(self.entry, v, self.kwargs, self.keep)
        ALIVE.append(c)
        return c

    def roles(self):
        return [(n, r, self.values[n]) for n, r in ENTRIES[self.entry][1]]

    def bufs(self):
        """every device buffer the call touches: (label, role, Buf); the items of a pointer table carry the table's role"""
        out = []
        for n, r, v in self.roles():
            if isinstance(v, Buf):
                out.append((n, r, v))
            elif isinstance(v, Table) and v.kind == "ptr":
                out += [("%s[%d]" % (n, i), r, b) for i, b in enumerate(v.items) if b is not None]
        return out

    def reset(self):
        for _, r, b in self.bufs():
            if r in (OUT, SCRATCH):
                fill_canary(b.t)
            elif b.snap is not None:
                b.t.copy_(b.snap)

    def launch(self):
        from dpf_nets_amd._lib import lib, current_stream
        args = [v.t.data_ptr() if isinstance(v, Buf) else v.c if isinstance(v, Table) else v for v in self.values.values()]
        return int(getattr(lib(), self.entry)(*args, current_stream()))

    def invoke(self):
        """reset, call, and wait: the next call may evict and destroy an executable graph, so nothing is left in flight"""
        import torch
        self.reset()
        torch.cuda.synchronize()
        rc = self.launch()
        torch.cuda.synchronize()
        return rc

    def outputs(self):
        """{label: bytes} of everything the call leaves behind for its caller"""
        return {n: b.bytes().clone() for n, r, b in self.bufs() if r in (OUT, INOUT) or b.snap is not None}

    def contents(self):
        """what load() needs to put this call's inputs back"""
        return [(b, b.t.clone(), None if b.snap is None else b.snap.clone()) for _, r, b in self.bufs() if r not in (OUT, SCRATCH)]

    def load(self, other):
        """copy the inputs of `other` (same entry, no larger) to the front of this call's buffers"""
        mine = {n: b for n, r, b in self.bufs() if r not in (OUT, SCRATCH)}
        for n, r, b in other.bufs():
            if r in (OUT, SCRATCH):
                continue
            dst = mine[n]
            nb = b.bytes().numel()
            assert nb <= dst.bytes().numel(), (n, nb, dst.bytes().numel())
            dst.bytes()[:nb].copy_(b.bytes())
            if dst.snap is not None:
                import torch
                dst.snap.view(torch.uint8).reshape(-1)[:nb].copy_(b.snap.view(torch.uint8).reshape(-1))


def restore(contents):
    for b, t, snap in contents:
        b.t.copy_(t)
        if snap is not None:
            b.snap.copy_(snap)


def stats():
    """(replays, eager, records, evictions, uncapturable), process-wide"""
    from dpf_nets_amd._lib import lib
    out = (ctypes.c_long * 5)()
    lib().dpf_train_graph_stats(out)
    return tuple(int(v) for v in out)


def set_enabled(on):
    from dpf_nets_amd._lib import lib
    return int(lib().dpf_train_graph_set_enabled(1 if on else 0))


def reference(call):
    """(return code, outputs) of the same entry with the same arguments with recording switched off"""
    prev = set_enabled(0)
    try:
        rc = call.invoke()
        return rc, call.outputs()
    finally:
        set_enabled(prev)


# ---- builders (GPU) ------------------------------------------------------------------------------------------------------
G = 64


def _decoder_blocks(seed, n_layers, B, N, mode, train):
    """a seeded LocalCondRNVPDecoder(1, 64, 64), the StackSpec of its first n_layers layers, the parameter blocks of the C ABI
    (as test_c_abi_backward_block_form_equals_the_pointer_list_form gathers them) and the inputs"""
    import torch
    from oracle import flow_oracle as FO
    from dpf_nets_amd import networks as nets
    from dpf_nets_amd.networks import train_engine as TE
    torch.manual_seed(1000 + seed)
    dec = nets.LocalCondRNVPDecoder(1, 64, G, weight_std=0.02).cuda()
    dec = dec.train() if train else dec.eval()
    layers = dec.coupling_layers()[:n_layers]
    spec = TE.StackSpec(layers)
    L, K = spec.L, 4 * spec.L
    if not train:                                                # frozen statistics of the set's own, not the initial 0 / 1
        with torch.no_grad():
            for bn in spec.flow_bns() + [m[1] for m in spec.film_modules()]:
                bn.running_mean.normal_(0.0, 0.1)
                bn.running_var.uniform_(0.5, 1.5)
    Bf = max(B, 2)                                              # the FiLM nets' batch-statistics BatchNorm needs two clouds
    tgt, z, g = FO.synthetic_inputs(seed, Bf, N, G)
    p = torch.from_numpy((tgt if mode == "inverse" else z).copy()).cuda()
    tg = torch.from_numpy(g.copy()).cuda()
    cp, fp = spec.canon_params(), spec.film_params()
    zeros = spec.zeros_on(p.device)
    with torch.no_grad():
        tcanon = torch.cat([cp[i].reshape(-1) if kind == "p" else zeros[:i] for kind, i in spec.cat_plan]).view(L, -1).contiguous()
        W0 = torch.cat([t.reshape(-1) for t in fp[0::5]]).view(K, 64, G)
        gam, bet = torch.cat(fp[1::5]).view(K, 1, 64), torch.cat(fp[2::5]).view(K, 1, 64)
        W1, b1 = torch.cat([t.reshape(-1) for t in fp[3::5]]).view(K, 64, 64), torch.cat(fp[4::5]).view(K, 1, 64)
    return dec, layers, spec, p, tg, tcanon, (W0, gam, bet, W1, b1)


def _gradients(seed, shape, table):
    import torch
    gen = torch.Generator(device="cuda").manual_seed(seed)
    blocks = [torch.randn(shape, device="cuda", generator=gen) * s for s in (1.0, 0.3, 0.1)]
    if not table:
        return [Buf(b) for b in blocks]
    return [Table("ptr", [Buf(b[i]) for i in range(shape[0])]) for b in blocks]


def _stack_tail(L, B, p, tcanon, eps, ws_bytes):
    import torch
    e = lambda *shape: torch.empty(shape, dtype=torch.float32, device="cuda")     # noqa: E731
    return {"dp_in": Buf(torch.empty_like(p)), "dp_tmp": Buf(torch.empty_like(p)), "dcanon": Buf(torch.empty_like(tcanon)),
            "dfm": Buf(e(L, 2, 2, B, 64)), "flow_eps": eps, "workspace": Buf(torch.empty(ws_bytes, dtype=torch.uint8, device="cuda"))}


def _build_stack(entry, seed, n_layers, B, N, mode, precision, flow_eps):
    import torch
    from dpf_nets_amd._lib import lib, check, current_stream, PREC, MODE
    L_ = lib()
    dec, layers, spec, p, tg, tcanon, (W0, gam, bet, W1, b1) = _decoder_blocks(seed, n_layers, B, N, mode, True)
    L, K, Bf, prec = spec.L, 4 * spec.L, p.shape[0], PREC[precision]
    eps = spec.eps * 2 if flow_eps == "double" else spec.eps
    e = lambda *shape: torch.empty(shape, dtype=torch.float32, device="cuda")     # noqa: E731
    # the 4 L FiLM nets, as train_engine._forward_core runs them, then the clouds of this call
    fm, xhat = e(L, 2, 2, Bf, 64), e(K, Bf, 64)
    rstd, fmean, fuvar = e(K, 64), e(K, 64), e(K, 64)
    check(L_.dpf_film_train_forward(K, Bf, G, tg.data_ptr(), W0.data_ptr(), gam.data_ptr(), bet.data_ptr(), W1.data_ptr(), b1.data_ptr(),
                                    float(spec.film_modules()[0][1].eps), fm.data_ptr(), xhat.data_ptr(), rstd.data_ptr(),
                                    fmean.data_ptr(), fuvar.data_ptr(), current_stream()), "film_train_forward")
    fm, p = fm[:, :, :, :B].contiguous(), p[:B].contiguous()
    packed = torch.empty(L_.dpf_flow_train_packed_bytes(L, prec), dtype=torch.uint8, device="cuda")
    check(L_.dpf_flow_train_pack(L, prec, tcanon.data_ptr(), packed.data_ptr(), current_stream()), "flow_train_pack")
    torch.cuda.synchronize()
    ws_bytes = L_.dpf_flow_train_workspace_bytes(B, N)
    head = {"n_layers": L, "B": B, "N": N, "mode": MODE[mode], "precision": prec, "meta_host": Table("int", list(spec.meta_host))}
    fwd = dict(head)
    fwd.update({"meta_dev": Buf(spec.meta_on(p.device).clone()), "tcanon": Buf(tcanon), "packed": inout(packed), "fm": Buf(fm),
                "p_in": Buf(p), "ps": Buf(e(L, B, 3, N)), "mus": Buf(e(L, B, 3, N)), "logvars": Buf(e(L, B, 3, N)),
                "stats": Buf(e(L, L_.dpf_flow_train_stats_floats())), "film": Buf(e(L, L_.dpf_flow_train_film_floats(B))),
                "flow_eps": eps, "workspace": Buf(torch.empty(ws_bytes, dtype=torch.uint8, device="cuda"))})
    keep = (dec, spec, tg, W0, gam, bet, W1, b1, xhat)
    forward = Call("dpf_flow_train_forward", fwd, keep=keep)
    if entry == "dpf_flow_train_forward":
        return forward
    rc, _ = reference(forward)                                   # the state the backward reads, left in the forward's buffers
    check(rc, "flow_train_forward")
    bwd = dict(head)
    bwd.update({"tcanon": fwd["tcanon"], "packed": Buf(fwd["packed"].t)})
    bwd.update({n: fwd[n] for n in ("film", "stats", "p_in", "ps", "mus", "logvars")})
    g_ps, g_mus, g_lvs = _gradients(seed, (L, B, 3, N), entry.endswith("_lists"))
    bwd.update({"g_ps": g_ps, "g_mus": g_mus, "g_lvs": g_lvs})
    bwd.update(_stack_tail(L, B, p, tcanon, eps, ws_bytes))
    return Call(entry, bwd, keep=(keep, forward))


def _build_frozen(entry, seed, n_layers, B, N, mode, precision, flow_eps):
    import torch
    from dpf_nets_amd._lib import lib, PREC, MODE
    from dpf_nets_amd.networks import frozen_engine as FZ
    from dpf_nets_amd.networks.engine import FlowStack
    dec, layers, spec, p, tg, tcanon, blocks = _decoder_blocks(seed, n_layers, B, N, mode, False)
    p, tg = p[:B].contiguous(), tg[:B].contiguous()
    stack = FlowStack(layers)
    with torch.no_grad():
        _, saved = FZ._forward_core(stack, spec, p, tg, mode, None, tcanon, *blocks)
    p_, g_, tcanon_, fstats, packed, film, fm, ps, mus, lvs = saved[:10]
    torch.cuda.synchronize()
    L = spec.L
    eps = spec.eps * 2 if flow_eps == "double" else spec.eps
    v = {"n_layers": L, "B": B, "N": N, "mode": MODE[mode], "precision": PREC[precision], "meta_host": Table("int", list(spec.meta_host)),
         "tcanon": Buf(tcanon), "fstats": Buf(fstats), "packed": Buf(packed.clone()), "film": Buf(film.clone()), "fm": Buf(fm),
         "p_in": Buf(p), "ps": Buf(ps.contiguous()), "mus": Buf(mus.contiguous()), "logvars": Buf(lvs.contiguous())}
    g_ps, g_mus, g_lvs = _gradients(seed, (L, B, 3, N), True)
    v.update({"g_ps": g_ps, "g_mus": g_mus, "g_lvs": g_lvs})
    v.update(_stack_tail(L, B, p, tcanon, eps, lib().dpf_flow_frozen_workspace_bytes(B, N)))
    return Call(entry, v, keep=(dec, spec, stack, saved, tg))


def _build_encoder(entry, seed, B, N, precision, momentum):
    """the arguments as networks/encoders.py's _TrainPool builds them, with batch_stats and non-trivial running statistics"""
    import torch
    from dpf_nets_amd._lib import lib, check, PREC
    from dpf_nets_amd import networks as nets
    L_ = lib()
    torch.manual_seed(2000 + seed)
    enc = nets.PointNetCloudEncoder(3, 64, [128, 256, 512]).cuda().train()
    gen = torch.Generator(device="cuda").manual_seed(seed)
    rnd = lambda *shape: torch.randn(shape, device="cuda", generator=gen)        # noqa: E731
    canon = torch.cat([t.detach().reshape(-1).to(torch.float32) for t in enc._layer_tensors()]).contiguous()
    x = rnd(B, 3, N)
    running = []
    for c in (64, 128, 256, 512):
        running += [inout(0.1 * rnd(c)), inout(1.0 + 0.5 * rnd(c).abs())]
    fwd = {"B": B, "N": N, "precision": PREC[precision], "canon": Buf(canon), "x": Buf(x),
           "ws": Buf(torch.empty(L_.dpf_encoder_train_workspace_bytes(B, N), dtype=torch.uint8, device="cuda")),
           "pooled": Buf(torch.empty((B, 512), dtype=torch.float32, device="cuda")),
           "batch_stats": Buf(torch.empty(2 * 960, dtype=torch.float32, device="cuda")), "running": Table("ptr", running),
           "momentum": momentum}
    forward = Call("dpf_encoder_train_forward", fwd, keep=enc)
    if entry == "dpf_encoder_train_forward":
        return forward
    rc, _ = reference(forward)                                   # leaves the step's state in ws
    check(rc, "encoder_train_forward")
    bwd = {"B": B, "N": N, "canon": fwd["canon"], "x": fwd["x"], "ws": inout(fwd["ws"].t), "pooled": Buf(fwd["pooled"].t),
           "g_pooled": Buf(rnd(B, 512)), "dcanon": Buf(torch.empty_like(canon)), "dx": Buf(torch.empty_like(x))}
    return Call(entry, bwd, keep=(enc, forward))


def build(entry, seed, **over):
    """A fresh argument set of `entry`: own weights, own inputs, own buffers, all derived from `seed`.  Built with recording
    off, so no counter moves and no cache slot is taken."""
    import torch
    fam = family(entry)
    kwargs = dict(BASE[fam])
    kwargs.update(over)
    prev = set_enabled(0)
    try:
        call = {"stack": _build_stack, "frozen": _build_frozen, "encoder": _build_encoder}[fam](entry, seed, **kwargs)
        torch.cuda.synchronize()
    finally:
        set_enabled(prev)
    call.kwargs = kwargs
    ALIVE.append(call)
    return call
