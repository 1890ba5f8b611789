"""Lazy list of per-layer (B,3,N) tensors backed by one (L,B,3,N) buffer.

LocalCondRNVPDecoder.forward must return three python-list-like objects of
3*n_flows tensors in DIRECT order (lib/networks/decoders.py:54-72) which the
callers index ([0], [-1]), concatenate with `+` / `+=` (lib/networks/models.py:
119-122,169-171,214-216) and pass to sum() (lib/networks/losses.py:13).  The
fused HIP stack writes each list into a single buffer; this sequence hands out
views on demand instead of materialising 189 tensor objects per call, and
remembers the layer-sum the kernel accumulated in registers."""
from collections.abc import Sequence


def tag_layer_sum(views, total):
    """Tag the tensors of `views` as one stack's whole list, and the last of them with their layer-sum `total` (None: not
    at hand), so that a python list that ENDS with them -- `[prior] + views` -- can still be recognised (tagged_tail).
    The tags hold no reference back to a list: no cycles.  Returns `views`."""
    token = object()
    for i, v in enumerate(views):
        v._dpf_pos = (token, i)
    if total is not None and views:
        views[-1]._dpf_total = (token, len(views), total)
    return views


def tagged_tail(logvars):
    """(k, total) when the last k entries of `logvars` are one stack's whole list whose layer-sum is `total`, else None."""
    n = len(logvars)
    tag = getattr(logvars[-1], "_dpf_total", None) if n else None
    if tag is not None:
        token, k, total = tag
        if n >= k and all(getattr(logvars[n - k + i], "_dpf_pos", None) == (token, i) for i in range(k)):
            return k, total
    return None


class FlowList(Sequence):
    def __init__(self, buf, total=None):
        self._buf = buf            # (L, B, 3, N)
        self._total = total        # (B, 3, N) = sum over L from the kernel, or None
        self._views = None

    def __len__(self):
        return self._buf.shape[0]

    def views(self):
        if self._views is None:
            # tagged: a python list built by `[prior] + flowlist` is still recognised by losses.total_logvar
            self._views = tag_layer_sum(list(self._buf.unbind(0)), self._total)
        return self._views

    def __getitem__(self, i):
        if isinstance(i, slice):
            return self.views()[i]
        if self._views is not None:
            return self._views[i]
        L = len(self)
        if not -L <= i < L:
            raise IndexError(i)
        return self._buf[i]

    def __iter__(self):
        return iter(self.views())

    def __add__(self, other):
        return self.views() + list(other)

    def __radd__(self, other):
        return list(other) + self.views()

    def total(self):
        if self._total is None:
            self._total = self._buf.sum(0)
        return self._total

    @property
    def stacked(self):
        return self._buf
