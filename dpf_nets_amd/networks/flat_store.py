"""ParamStore: the parameters of a stack of flow layers in ONE fp32 buffer, their gradients in its twin.

The base of train_engine.FlatStore (the point decoder) and prior_flows.PriorFlatStore (the latent prior flow); the
subclasses choose the layout (`slots`) and add what the kernels of their stack write.  Every nn.Parameter keeps its
identity, name and shape (state dicts and optimizers are unaffected); its `.data` becomes a view of `flat_p` and its
`.grad` a view of `flat_g`.

Gradients are written by the stack's autograd node itself (autograd sees only the inputs and `token`), so per-parameter
autograd hooks (and with them DistributedDataParallel's reducer) do not fire for these parameters: use
dpf_nets_amd.distributed.allreduce_flat_gradients.  `optimizer.zero_grad()` may set the grads to None; the next
backward re-attaches the views (zeroed) -- `zero_grad()` here avoids that per-parameter pass."""
import torch


def _mark_grad_written(p):
    st = getattr(p, "_dpf_flat", None)
    if st is not None:
        st.grad_written = True


def hook_grad_written(params):
    """`grad_written` is a HINT that the store's own writers keep up to date (accumulate, attach_grads, the exchanges);
    gradients that reach flat_g by ordinary autograd -- AccumulateGrad adding in place into the attached views: the
    tensor-op path of a flattened decoder (DPF_TRAIN_IMPL=torch, forward_torch), an eval-mode decoder under autograd,
    forward(n_layers=...), a single flow module's own forward -- set it through a post-accumulate hook on every parameter
    (registered once per Parameter object; the store is looked up at call time, so a rebuilt store is found).  The hooks
    never fire on the flat path, whose node writes flat_g itself."""
    for t in params:
        if not getattr(t, "_dpf_gw_hook", False):
            t.register_post_accumulate_grad_hook(_mark_grad_written)
            t._dpf_gw_hook = True


class ParamStore:
    def __init__(self, params, slots, total, device):
        """slots: the (offset, numel) of every parameter inside the `total` floats of the flat buffers."""
        self.params, self.slots, self.total = list(params), list(slots), total
        self.flat_p = torch.zeros(total, dtype=torch.float32, device=device)
        self.flat_g = torch.zeros_like(self.flat_p)
        with torch.no_grad():
            torch._foreach_copy_([self.flat_p[o:o + n] for o, n in self.slots], [t.detach().reshape(-1).to(device) for t in self.params])
        self.pviews, self.gviews = self.views_of(self.flat_p), self.views_of(self.flat_g)
        # a gradient was written into flat_g since the last zero_grad(set_to_none=True) -- what "p.grad is not None" means
        # for parameters whose .grad views stay attached (networks.optimizers.Adam skips a store without one)
        self.grad_written = any(t.grad is not None for t in self.params)
        for t, pv, gv in zip(self.params, self.pviews, self.gviews):
            if t.grad is not None:
                gv.copy_(t.grad)
            t.data = pv
            t.grad = gv
            t._dpf_flat = self              # networks.optimizers.Adam updates a whole store at once
        hook_grad_written(self.params)
        self.token = torch.zeros(1, dtype=torch.float32, device=device, requires_grad=True)

    def views_of(self, buf):
        """Every parameter's slice of `buf` (laid out as flat_p), in its shape."""
        return [buf[o:o + n].view(t.shape) for (o, n), t in zip(self.slots, self.params)]

    def attached(self):
        """The aliasing survives in-place updates, load_state_dict and optimizer steps; module.to()/.cuda()/.float()
        re-assign `.data` and break it (the module then builds a new store)."""
        a, b, pv = self.params[0], self.params[-1], self.pviews
        return a.data_ptr() == pv[0].data_ptr() and b.data_ptr() == pv[-1].data_ptr() and a.device == self.flat_p.device

    def grads_attached(self, full=False):
        """Every parameter's .grad is its view of flat_g.  The per-step check looks at three sentinel parameters only
        (first, middle, last); full=True examines all of them."""
        ps, gv, mid = self.params, self.gviews, len(self.params) // 2
        if full:
            return all(t.grad is v for t, v in zip(ps, gv))
        return ps[0].grad is gv[0] and ps[mid].grad is gv[mid] and ps[-1].grad is gv[-1]

    def rebase_grads(self, buf):
        """Move the gradient buffer onto `buf` (a contiguous fp32 slice of a bigger buffer, same length): contents carried
        over, every parameter's .grad re-pointed.  distributed.GradArena uses this to make the gradients of a whole model
        -- both stores, every other parameter -- ONE flat message."""
        assert buf.numel() == self.flat_g.numel() and buf.dtype == torch.float32 and buf.is_contiguous() and buf.device == self.flat_g.device
        with torch.no_grad():
            buf.copy_(self.flat_g)
        self.flat_g = buf
        self.gviews = self.views_of(buf)
        for t, gv in zip(self.params, self.gviews):
            t.grad = gv

    def zero_grad(self):
        self.flat_g.zero_()
        self.grad_written = False
        self.attach_grads(zeroed=True)

    def attach_grads(self, zeroed=False, full=False):
        """Make every parameter's .grad the view of flat_g again: after optimizer.zero_grad(set_to_none=True) the views
        come back zeroed; a .grad that was replaced by another tensor is copied in.  full=True walks all the parameters
        whatever the sentinels of grads_attached() say."""
        if not full and self.grads_attached():
            return
        ps, gv = self.params, self.gviews
        if not zeroed:
            if all(t.grad is None for t in ps):
                self.flat_g.zero_()
                self.grad_written = False
            else:
                self.grad_written = True
                for t, v in zip(ps, gv):
                    if t.grad is None:
                        v.zero_()
                    elif t.grad is not v:
                        v.copy_(t.grad)
        for t, v in zip(ps, gv):
            t.grad = v
