"""The recurrent core: the reference's PolicyRNN (scripts/jax_policy.py, make_policy: an LSTM of 256 hidden channels
and one layer, a LayerNorm on its output, clear_recurrent_state at episode ends) with everything after the two gate
GEMMs in one kernel, forward and backward (hs_lstm_cell, hs_lstm_cell_backward, csrc/hs_k_lstm.h).

The GEMMs gates = x W_in + h W_rec stay with torch (the matrix cores); the kernel adds the bias, applies the four gate
activations (order i, f, g, o), updates the cell, norms the output over the H channels and zeroes the carried state of
the rows whose episode just ended (`clear`: the simulator's done export).  include/hideseek.h states the arithmetic, IEEE
f32 in a fixed order.  y is the LayerNorm of the uncleared output: the clear applies to the carried state alone.
madrona_learn's LSTM is not part of the reference's tree, so gate order, eps and the place of the clear are the project's.

    core = recurrent.LSTMCore(in_features=256, hidden=256).cuda()      # w_in [F, 4H], w_rec [H, 4H], cell_params [6H]
    state = core.init_state(rows, "cuda", torch.bfloat16)              # (h in the GEMM's dtype, c float32)
    for t in range(T):                                                 # the rollout
        sim.step()
        y, state = core(sim, feats[t], state, clear=sim.done_tensor().to_torch().reshape(rows))
    ys, state = core.sequence(sim, xs, state0, clears)                 # a training chunk: autograd runs through time
    loss(ys).backward()                                                # the backward kernel per step, torch for the GEMMs

or without autograd: sim.lstm_cell(gates, c_prev, core.cell_params.detach(), clear=done, y=y_buf[t]).  eager() is the
same composition in plain torch, for readers, tools/lstm_bench.py and the tests.
"""
import ctypes as C
import functools

from ._request import _DTYPES, _above_zero, _dtype_arg, _module_base, _name, _one_of, _outputs, _run, _shard_calls, _tensor, _vector, _wanted

HIDDEN = (64, 128, 256, 512)
PARAM_ROWS = 6            # HS_LSTM_PARAM_ROWS: bias i, f, g, o | gamma | beta, rows of H floats
MAX_GRID_BWD = 512        # HS_LSTM_MAX_GRID_BWD: workgroups (and workspace slices) of a backward call at the most
ROWS_PER_ROUND = 4        # HS_LSTM_ROWS_PER_ROUND: one row per wave, four waves
SUM_SEGS = 8              # HS_EMBED_SUM_SEGS: the slices are added by the encoder's sum kernel
GATES = ("i", "f", "g", "o")
DEFAULT_EPS = 1e-6        # flax's LayerNorm epsilon


class HsLstmCellRequest(C.Structure):
    """hs_lstm_cell_request (include/hideseek.h)."""
    _fields_ = [("gates", C.c_void_p), ("c_prev", C.c_void_p), ("cell_params", C.c_void_p), ("clear", C.c_void_p), ("n", C.c_int32),
                ("hidden", C.c_int32), ("gates_dtype", C.c_int32), ("y_dtype", C.c_int32), ("eps", C.c_float), ("reserved", C.c_int32),
                ("y", C.c_void_p), ("h_next", C.c_void_p), ("c_next", C.c_void_p)]


class HsLstmCellBackwardRequest(C.Structure):
    """hs_lstm_cell_backward_request (include/hideseek.h)."""
    _fields_ = [("gates", C.c_void_p), ("c_prev", C.c_void_p), ("cell_params", C.c_void_p), ("clear", C.c_void_p), ("grad_y", C.c_void_p),
                ("grad_h_next", C.c_void_p), ("grad_c_next", C.c_void_p), ("n", C.c_int32), ("hidden", C.c_int32), ("gates_dtype", C.c_int32),
                ("y_dtype", C.c_int32), ("eps", C.c_float), ("reserved", C.c_int32), ("grad_gates", C.c_void_p), ("grad_c_prev", C.c_void_p),
                ("grad_cell_params", C.c_void_p)]


# ---- the parameters ----
def _hidden(H):
    return _one_of("hidden", H, HIDDEN)


def param_layout(H):
    """{"bias": (first, one past the last, (4, H)), "scale": (.., (H,)), "shift": (.., (H,))}: the element ranges of the
    flat cell_params tensor of PARAM_ROWS * H float32; row k of bias belongs to gate GATES[k]."""
    H = _hidden(H)
    return {"bias": (0, 4 * H, (4, H)), "scale": (4 * H, 5 * H, (H,)), "shift": (5 * H, 6 * H, (H,))}


def views(cell_params, H):
    """The named zero-copy views of a flat cell_params (or gradient) tensor after param_layout."""
    if cell_params.dim() != 1 or cell_params.numel() != PARAM_ROWS * _hidden(H):
        raise ValueError(f"cell_params must have shape ({PARAM_ROWS * H},), got {tuple(cell_params.shape)}")
    return {k: cell_params[lo:hi].view(sh) for k, (lo, hi, sh) in param_layout(H).items()}


def init_cell_params(H):
    """Fresh flat float32 cell_params (on the CPU): biases 0, LayerNorm scale 1 and shift 0."""
    import torch
    p = torch.zeros(PARAM_ROWS * _hidden(H), dtype=torch.float32)
    views(p, H)["scale"].fill_(1.0)
    return p


def eager(gates, c_prev, cell_params, clear=None, eps=DEFAULT_EPS):
    """The plain-torch composition in the dtype of c_prev (float32, or float64 for a reference): (y, h_next, c_next) of
    gates [n, 4H], c_prev [n, H], cell_params [6H] and clear [n] (integers, nonzero = zero the carried state) or None.
    Differentiable in gates, c_prev and cell_params."""
    import torch
    H = c_prev.shape[-1]
    ft = c_prev.dtype
    p = views(cell_params.to(ft), H)
    zi, zf, zg, zo = (gates.to(ft).view(-1, 4, H) + p["bias"]).unbind(1)
    i, f, g, o = torch.sigmoid(zi), torch.sigmoid(zf), torch.tanh(zg), torch.sigmoid(zo)
    c = f * c_prev + i * g
    h = o * torch.tanh(c)
    y = torch.nn.functional.layer_norm(h, (H,), p["scale"], p["shift"], eps)
    if clear is not None:
        keep = (clear.reshape(-1, 1) == 0)
        h, c = torch.where(keep, h, torch.zeros_like(h)), torch.where(keep, c, torch.zeros_like(c))
    return y, h, c


def eager_sequence(xs, w_in, w_rec, cell_params, state, clears=None, eps=DEFAULT_EPS):
    """LSTMCore.sequence in plain torch, in the dtype of the state's c: ys [T, n, H] and the final (h, c)."""
    import torch
    h, c = state
    ys = []
    for t in range(xs.shape[0]):
        gates = torch.addmm(xs[t].to(c.dtype) @ w_in.to(c.dtype), h.to(c.dtype), w_rec.to(c.dtype))
        y, h, c = eager(gates, c, cell_params, None if clears is None else clears[t], eps)
        ys.append(y)
    return torch.stack(ys), (h, c)


# ---- the fused calls ----
def _common(gpu_id, gates, c_prev, cell_params, clear, hidden, eps):
    import torch
    dev = torch.device("cuda", gpu_id)
    if hidden is None and isinstance(c_prev, torch.Tensor) and c_prev.dim() == 2:
        hidden = int(c_prev.shape[1])
    H = _hidden(hidden)
    e = _above_zero("eps", eps)
    _tensor("gates", gates, ("n >= 1", 4 * H), _DTYPES, dev, bound=4 * H)
    n = int(gates.shape[0])
    _tensor("c_prev", c_prev, (n, H), ("float32",), dev)
    _tensor("cell_params", cell_params, (PARAM_ROWS * H,), ("float32",), dev)
    inputs = [("gates", gates), ("c_prev", c_prev), ("cell_params", cell_params)]
    if clear is not None:
        _vector("clear", clear, n, dev, ("int32",), "None or a torch tensor")
        inputs.append(("clear", clear))
    return dev, H, n, e, inputs


def request(gpu_id, gates, c_prev, cell_params, clear=None, hidden=None, eps=DEFAULT_EPS, y=True, h_next=True, c_next=True, y_dtype=None):
    """Validate a forward call over the n = gates.shape[0] rows on GPU `gpu_id` (hidden defaults to c_prev's width),
    allocate the outputs given as True (y in `y_dtype`, by default the dtype of the gates; h_next in the gates' dtype;
    c_next float32), and return ({name: tensor}, HsLstmCellRequest).  Raises ValueError before the library is involved."""
    import torch
    dev, H, n, eps, inputs = _common(gpu_id, gates, c_prev, cell_params, clear, hidden, eps)
    outputs = _wanted((("y", y), ("h_next", h_next), ("c_next", c_next)), "none of y, h_next and c_next requested")
    _dtype_arg("y_dtype", y_dtype)
    specs = {"y": ((n, H), gates.dtype if y_dtype is None else y_dtype, _DTYPES), "h_next": ((n, H), gates.dtype),
             "c_next": ((n, H), torch.float32)}
    res, ptr = _outputs(outputs, specs, inputs, dev)
    req = HsLstmCellRequest(gates.data_ptr(), c_prev.data_ptr(), cell_params.data_ptr(), None if clear is None else clear.data_ptr(), n, H,
                            _DTYPES[_name(gates.dtype)], _DTYPES[_name(res["y"].dtype)] if "y" in res else 0, eps, 0, ptr("y"), ptr("h_next"),
                            ptr("c_next"))
    return res, req


def request_backward(gpu_id, gates, c_prev, cell_params, grad_y, clear=None, grad_h_next=None, grad_c_next=None, hidden=None, eps=DEFAULT_EPS,
                     grad_gates=True, grad_c_prev=True, grad_cell_params=True):
    """Validate a backward call, allocate the outputs given as True (grad_gates in the gates' dtype, the others
    float32), and return ({name: tensor}, HsLstmCellBackwardRequest).  grad_y is float32, bfloat16 or float16 (the dtype
    of the forward's y), grad_h_next (or None = zero) has the gates' dtype and grad_c_next (or None) is float32.  Raises
    ValueError before the library is involved."""
    import torch
    dev, H, n, eps, inputs = _common(gpu_id, gates, c_prev, cell_params, clear, hidden, eps)
    gname = _name(gates.dtype)
    _tensor("grad_y", grad_y, (n, H), _DTYPES, dev)
    inputs.append(("grad_y", grad_y))
    for k, t, dts in (("grad_h_next", grad_h_next, (gname,)), ("grad_c_next", grad_c_next, ("float32",))):
        if t is not None:
            _tensor(k, t, (n, H), dts, dev, "None or a torch tensor")
            inputs.append((k, t))
    outputs = _wanted((("grad_gates", grad_gates), ("grad_c_prev", grad_c_prev), ("grad_cell_params", grad_cell_params)),
                      "none of grad_gates, grad_c_prev and grad_cell_params requested")
    specs = {"grad_gates": ((n, 4 * H), gates.dtype), "grad_c_prev": ((n, H), torch.float32),
             "grad_cell_params": ((PARAM_ROWS * H,), torch.float32)}
    res, ptr = _outputs(outputs, specs, inputs, dev)
    opt = lambda t: None if t is None else t.data_ptr()                        # noqa: E731
    req = HsLstmCellBackwardRequest(gates.data_ptr(), c_prev.data_ptr(), cell_params.data_ptr(), opt(clear), grad_y.data_ptr(), opt(grad_h_next),
                                    opt(grad_c_next), n, H, _DTYPES[gname], _DTYPES[_name(grad_y.dtype)], eps, 0, ptr("grad_gates"),
                                    ptr("grad_c_prev"), ptr("grad_cell_params"))
    return res, req


def compute(sim, gates, c_prev, cell_params, stream=None, **kw):
    """HideAndSeekSimulator.lstm_cell."""
    res, req = request(sim.gpu_id, gates, c_prev, cell_params, **kw)
    _run(sim, "hs_lstm_cell", req, stream)
    return res


def compute_backward(sim, gates, c_prev, cell_params, grad_y, stream=None, **kw):
    """HideAndSeekSimulator.lstm_cell_backward."""
    res, req = request_backward(sim.gpu_id, gates, c_prev, cell_params, grad_y, **kw)
    _run(sim, "hs_lstm_cell_backward", req, stream)
    return res


def compute_sharded(ssim, gates, c_prev, cell_params, stream=None, clear=None, y=True, h_next=True, c_next=True, **kw):
    """ShardedSimulator.lstm_cell: every shard works its own rows on its own device."""
    return _shard_calls(ssim, "hs_lstm_cell", request, stream, dict(gates=gates, c_prev=c_prev), dict(cell_params=cell_params),
                        dict(clear=clear, y=y, h_next=h_next, c_next=c_next), kw)


def compute_backward_sharded(ssim, gates, c_prev, cell_params, grad_y, stream=None, clear=None, grad_h_next=None, grad_c_next=None,
                             grad_gates=True, grad_c_prev=True, grad_cell_params=True, **kw):
    """ShardedSimulator.lstm_cell_backward: as compute_sharded; every shard's grad_cell_params holds the sum over its own
    rows (add them for shared parameters)."""
    return _shard_calls(ssim, "hs_lstm_cell_backward", request_backward, stream, dict(gates=gates, c_prev=c_prev, grad_y=grad_y),
                        dict(cell_params=cell_params), dict(clear=clear, grad_h_next=grad_h_next, grad_c_next=grad_c_next, grad_gates=grad_gates,
                                                            grad_c_prev=grad_c_prev, grad_cell_params=grad_cell_params), kw)


# ---- the autograd face ----
@functools.lru_cache(maxsize=None)
def _function():
    import torch

    class _Cell(torch.autograd.Function):
        @staticmethod
        def forward(ctx, gates, c_prev, cell_params, sim, clear, eps):
            gates, c_prev = gates.detach().contiguous(), c_prev.detach().contiguous()
            out = compute(sim, gates, c_prev, cell_params.detach(), clear=clear, eps=eps)
            ctx.save_for_backward(gates, c_prev, cell_params)
            ctx.call = (sim, clear, eps)
            return out["y"], out["h_next"], out["c_next"]

        @staticmethod
        def backward(ctx, grad_y, grad_h, grad_c):
            gates, c_prev, cell_params = ctx.saved_tensors
            sim, clear, eps = ctx.call
            grad_y = torch.zeros_like(gates[:, :c_prev.shape[1]]) if grad_y is None else grad_y.contiguous()
            res = compute_backward(sim, gates, c_prev, cell_params.detach(), grad_y, clear=clear, eps=eps,
                                   grad_h_next=None if grad_h is None else grad_h.contiguous(),
                                   grad_c_next=None if grad_c is None else grad_c.contiguous(),
                                   grad_gates=ctx.needs_input_grad[0] or None, grad_c_prev=ctx.needs_input_grad[1] or None,
                                   grad_cell_params=ctx.needs_input_grad[2] or None)
            return res.get("grad_gates"), res.get("grad_c_prev"), res.get("grad_cell_params"), None, None, None
    return _Cell


class LSTMCore(_module_base()):
    """PolicyRNN as a torch module: float32 Parameters w_in [F, 4H] and w_rec [H, 4H] (orthogonal) and one flat
    cell_params [6H] (biases 0, scale 1, shift 0; named_views() gives bias [4, H], scale and shift as views).
    forward(sim, x, state, clear) computes the gates with torch.addmm in the dtype of the state's h and runs the fused
    cell on `sim`'s device as part of the autograd graph: its backward is the backward kernel, which hands torch the
    gradients of the gates, of c_prev and of cell_params, so w_in, w_rec, x and the previous step get theirs from torch.
    `clear` gets no gradient."""

    def __init__(self, in_features, hidden=256, eps=DEFAULT_EPS, generator=None):
        import torch
        super().__init__()
        if isinstance(in_features, bool) or not isinstance(in_features, int) or in_features < 1:
            raise ValueError(f"in_features must be a positive integer, got {in_features}")
        self.in_features, self.hidden, self.eps = in_features, _hidden(hidden), float(eps)
        self.w_in = torch.nn.Parameter(torch.nn.init.orthogonal_(torch.empty(in_features, 4 * hidden), generator=generator))
        self.w_rec = torch.nn.Parameter(torch.nn.init.orthogonal_(torch.empty(hidden, 4 * hidden), generator=generator))
        self.cell_params = torch.nn.Parameter(init_cell_params(hidden))

    def named_views(self):
        return views(self.cell_params, self.hidden)

    def init_state(self, n, device, dtype=None):
        """(h [n, H] zeros in `dtype` (the GEMM's; float32 by default), c [n, H] float32 zeros)."""
        import torch
        return (torch.zeros(n, self.hidden, dtype=torch.float32 if dtype is None else dtype, device=device),
                torch.zeros(n, self.hidden, dtype=torch.float32, device=device))

    def forward(self, sim, x, state, clear=None):
        import torch
        h, c = state
        gates = torch.addmm(x.to(h.dtype) @ self.w_in.to(h.dtype), h, self.w_rec.to(h.dtype))
        y, h_next, c_next = _function().apply(gates, c, self.cell_params, sim, None if clear is None else clear.detach(), self.eps)
        return y, (h_next, c_next)

    def sequence(self, sim, xs, state, clears=None):
        """The loop over the T steps of a chunk: xs [T, n, F], clears [T, n] int32 or None (clears[t] is the done export
        of step t) -> ys [T, n, H] and the final state."""
        import torch
        ys = []
        for t in range(xs.shape[0]):
            y, state = self.forward(sim, xs[t], state, None if clears is None else clears[t])
            ys.append(y)
        return torch.stack(ys), state
