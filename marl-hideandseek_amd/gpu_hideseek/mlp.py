"""The MLP at the end of the reference's SimpleNet (scripts/jax_policy.py:163-167, MLP(num_channels=256, num_layers=3)):
per layer a Dense, a LayerNorm and a leaky ReLU, with everything after the GEMM in one kernel, forward and backward
(hs_dense_norm_act, hs_dense_norm_act_backward, csrc/hs_k_dense.h).

The GEMM z = x W stays with torch (the matrix cores), without the bias; the kernel adds the bias, norms over the C
channels and applies the leaky ReLU.  include/hideseek.h states the arithmetic, IEEE f32 in a fixed order.  madrona_learn's
MLP is not part of the reference's tree, so eps, slope and the he-normal initialiser are the project's (flax's defaults).

    net = mlp.MLP(in_features=256, channels=256, layers=3).cuda()      # per layer weight [in, C] and params [3 C]
    y = net(sim, feats)                                                # [n, 256] in feats' dtype, part of the autograd graph
    loss(y).backward()                                                 # the backward kernel per layer, torch for the GEMMs

or without autograd: sim.dense_norm_act(z, layer.params.detach(), y=y_buf).  eager() is the same composition in plain
torch, for readers, tools/mlp_bench.py and the tests; MLP(..., fused=False) runs it on the same parameters.

The kernel reads and writes a lane's adjacent channels as one piece of up to 16 bytes, so z, y, grad_y and grad_z must
be 16-byte aligned: any contiguous [n, C] view that starts at a row boundary of a torch allocation is.
"""
import ctypes as C
import functools
import math

from ._request import _DTYPES, _OUTPUT, _above_zero, _dtype_arg, _module_base, _name, _one_of, _outputs, _run, _shard_calls, _tensor, _wanted

CHANNELS = (64, 128, 256, 512)
PARAM_ROWS = 3            # HS_DENSE_PARAM_ROWS: bias | gamma | beta, rows of C floats
MAX_GRID_BWD = 512        # HS_DENSE_MAX_GRID_BWD: workgroups (and workspace slices) of a backward call at the most
ROWS_PER_ROUND = 4        # HS_DENSE_ROWS_PER_ROUND: one row per wave, four waves
SUM_SEGS = 8              # HS_EMBED_SUM_SEGS: the slices are added by the encoder's sum kernel
ALIGN = 16                # bytes: z, y, grad_y and grad_z
DEFAULT_EPS = 1e-6        # flax's LayerNorm epsilon
DEFAULT_SLOPE = 0.01      # flax's leaky_relu negative_slope


class HsDenseNormActRequest(C.Structure):
    """hs_dense_norm_act_request (include/hideseek.h)."""
    _fields_ = [("z", C.c_void_p), ("params", C.c_void_p), ("n", C.c_int32), ("channels", C.c_int32), ("z_dtype", C.c_int32),
                ("y_dtype", C.c_int32), ("eps", C.c_float), ("slope", C.c_float), ("y", C.c_void_p)]


class HsDenseNormActBackwardRequest(C.Structure):
    """hs_dense_norm_act_backward_request (include/hideseek.h)."""
    _fields_ = [("z", C.c_void_p), ("params", C.c_void_p), ("grad_y", C.c_void_p), ("n", C.c_int32), ("channels", C.c_int32),
                ("z_dtype", C.c_int32), ("y_dtype", C.c_int32), ("eps", C.c_float), ("slope", C.c_float), ("grad_z", C.c_void_p),
                ("grad_params", C.c_void_p)]


# ---- the parameters ----
def _channels(Cn):
    return _one_of("channels", Cn, CHANNELS)


def param_layout(Cn):
    """{"bias": (first, one past the last, (C,)), "scale": .., "shift": ..}: the element ranges of the flat params tensor
    of PARAM_ROWS * C float32."""
    Cn = _channels(Cn)
    return {"bias": (0, Cn, (Cn,)), "scale": (Cn, 2 * Cn, (Cn,)), "shift": (2 * Cn, 3 * Cn, (Cn,))}


def views(params, Cn):
    """The named zero-copy views of a flat params (or gradient) tensor after param_layout."""
    if params.dim() != 1 or params.numel() != PARAM_ROWS * _channels(Cn):
        raise ValueError(f"params must have shape ({PARAM_ROWS * Cn},), got {tuple(params.shape)}")
    return {k: params[lo:hi].view(sh) for k, (lo, hi, sh) in param_layout(Cn).items()}


def init_params(Cn):
    """Fresh flat float32 params (on the CPU): bias 0, LayerNorm scale 1 and shift 0."""
    import torch
    p = torch.zeros(PARAM_ROWS * _channels(Cn), dtype=torch.float32)
    views(p, Cn)["scale"].fill_(1.0)
    return p


def eager(z, params, eps=DEFAULT_EPS, slope=DEFAULT_SLOPE):
    """The plain-torch composition in the dtype of params (float32, or float64 for a reference): y [n, C] of z [n, C]
    (the GEMM's result without the bias) and params [3 C].  Differentiable in z and params."""
    import torch
    Cn = z.shape[-1]
    p = views(params, Cn)
    u = torch.nn.functional.layer_norm(z.to(params.dtype) + p["bias"], (Cn,), p["scale"], p["shift"], eps)
    return torch.nn.functional.leaky_relu(u, slope)


# ---- the fused calls ----
def _common(gpu_id, z, params, channels, eps, slope):
    import torch
    dev = torch.device("cuda", gpu_id)
    if not isinstance(z, torch.Tensor):
        raise ValueError("z must be a torch tensor")
    if channels is None:
        if z.dim() != 2:
            raise ValueError(f"z must be a tensor of shape (n >= 1, channels): its shape is {tuple(z.shape)}")
        channels = int(z.shape[1])
    Cn = _channels(channels)
    e, sl = _above_zero("eps", eps), float(slope)
    if not math.isfinite(sl) or not 0.0 <= C.c_float(sl).value <= 1.0:
        raise ValueError(f"slope must be finite and in [0, 1], got {slope}")
    _tensor("z", z, ("n >= 1", Cn), _DTYPES, dev, bound=Cn, align=ALIGN)
    _tensor("params", params, (PARAM_ROWS * Cn,), ("float32",), dev)
    return dev, Cn, int(z.shape[0]), e, sl, [("z", z), ("params", params)]


def _aligned_rows(n, Cn, dtypes, dev):
    """The checker of a [n, C] output: the plain one, plus the alignment the kernel's accesses need."""
    return lambda k, t: _tensor(k, t, (n, Cn), dtypes, dev, _OUTPUT, align=ALIGN)


def request(gpu_id, z, params, channels=None, eps=DEFAULT_EPS, slope=DEFAULT_SLOPE, y=True, y_dtype=None):
    """Validate a forward call over the n = z.shape[0] rows on GPU `gpu_id` (channels defaults to z's width), allocate y
    when given as True (in `y_dtype`, by default the dtype of z), and return ({"y": tensor}, HsDenseNormActRequest).
    Raises ValueError before the library is involved."""
    dev, Cn, n, eps, slope, inputs = _common(gpu_id, z, params, channels, eps, slope)
    outputs = _wanted((("y", y),), "y not requested")
    _dtype_arg("y_dtype", y_dtype)
    res, ptr = _outputs(outputs, {"y": ((n, Cn), z.dtype if y_dtype is None else y_dtype, _aligned_rows(n, Cn, _DTYPES, dev))}, inputs, dev)
    req = HsDenseNormActRequest(z.data_ptr(), params.data_ptr(), n, Cn, _DTYPES[_name(z.dtype)], _DTYPES[_name(res["y"].dtype)], eps, slope, ptr("y"))
    return res, req


def request_backward(gpu_id, z, params, grad_y, channels=None, eps=DEFAULT_EPS, slope=DEFAULT_SLOPE, grad_z=True, grad_params=True):
    """Validate a backward call, allocate the outputs given as True (grad_z in z's dtype, grad_params float32), and
    return ({name: tensor}, HsDenseNormActBackwardRequest).  grad_y is float32, bfloat16 or float16 (the dtype of the
    forward's y).  Raises ValueError before the library is involved."""
    import torch
    dev, Cn, n, eps, slope, inputs = _common(gpu_id, z, params, channels, eps, slope)
    _tensor("grad_y", grad_y, (n, Cn), _DTYPES, dev, align=ALIGN)
    inputs.append(("grad_y", grad_y))
    outputs = _wanted((("grad_z", grad_z), ("grad_params", grad_params)), "neither grad_z nor grad_params requested")
    specs = {"grad_z": ((n, Cn), z.dtype, _aligned_rows(n, Cn, (_name(z.dtype),), dev)),
             "grad_params": ((PARAM_ROWS * Cn,), torch.float32)}
    res, ptr = _outputs(outputs, specs, inputs, dev)
    req = HsDenseNormActBackwardRequest(z.data_ptr(), params.data_ptr(), grad_y.data_ptr(), n, Cn, _DTYPES[_name(z.dtype)],
                                        _DTYPES[_name(grad_y.dtype)], eps, slope, ptr("grad_z"), ptr("grad_params"))
    return res, req


def compute(sim, z, params, stream=None, **kw):
    """HideAndSeekSimulator.dense_norm_act."""
    res, req = request(sim.gpu_id, z, params, **kw)
    _run(sim, "hs_dense_norm_act", req, stream)
    return res


def compute_backward(sim, z, params, grad_y, stream=None, **kw):
    """HideAndSeekSimulator.dense_norm_act_backward."""
    res, req = request_backward(sim.gpu_id, z, params, grad_y, **kw)
    _run(sim, "hs_dense_norm_act_backward", req, stream)
    return res


def compute_sharded(ssim, z, params, stream=None, y=True, **kw):
    """ShardedSimulator.dense_norm_act: every shard works its own rows on its own device."""
    return _shard_calls(ssim, "hs_dense_norm_act", request, stream, dict(z=z), dict(params=params), dict(y=y), kw)


def compute_backward_sharded(ssim, z, params, grad_y, stream=None, grad_z=True, grad_params=True, **kw):
    """ShardedSimulator.dense_norm_act_backward: as compute_sharded; every shard's grad_params holds the sum over its own
    rows (add them for shared parameters)."""
    return _shard_calls(ssim, "hs_dense_norm_act_backward", request_backward, stream, dict(z=z, grad_y=grad_y), dict(params=params),
                        dict(grad_z=grad_z, grad_params=grad_params), kw)


# ---- the autograd face ----
def _aligned(t):
    """t, contiguous and ALIGN-byte aligned: itself where it already is (what torch's GEMMs and autograd hand over), else a copy."""
    t = t.contiguous()
    return t.clone() if t.data_ptr() % ALIGN else t


@functools.lru_cache(maxsize=None)
def _function():
    import torch

    class _DenseNormAct(torch.autograd.Function):
        @staticmethod
        def forward(ctx, z, params, sim, eps, slope):
            z = _aligned(z.detach())
            out = compute(sim, z, params.detach(), eps=eps, slope=slope)
            ctx.save_for_backward(z, params)
            ctx.call = (sim, eps, slope)
            return out["y"]

        @staticmethod
        def backward(ctx, grad_y):
            z, params = ctx.saved_tensors
            sim, eps, slope = ctx.call
            res = compute_backward(sim, z, params.detach(), _aligned(grad_y), eps=eps, slope=slope,
                                   grad_z=ctx.needs_input_grad[0] or None, grad_params=ctx.needs_input_grad[1] or None)
            return res.get("grad_z"), res.get("grad_params"), None, None, None
    return _DenseNormAct


class DenseNormAct(_module_base()):
    """One layer as a torch module: a float32 Parameter weight [in_features, C] (he-normal, flax MLP's usual initialiser:
    the project's choice, not pinned by the reference) and one flat params [3 C] (bias 0, scale 1, shift 0; named_views()
    gives them as views).  forward(sim, x) computes z = x.to(dt) @ weight.to(dt) in x's dtype dt and runs the fused call
    on `sim`'s device as part of the autograd graph: its backward is the backward kernel, which hands torch the gradients
    of z and of params, so weight and x get theirs from torch.  With fused=False the call is eager() on the same
    parameters (then `sim` is not used and may be None)."""

    def __init__(self, in_features, channels=256, eps=DEFAULT_EPS, slope=DEFAULT_SLOPE, fused=True, generator=None):
        import torch
        super().__init__()
        if isinstance(in_features, bool) or not isinstance(in_features, int) or in_features < 1:
            raise ValueError(f"in_features must be a positive integer, got {in_features}")
        self.in_features, self.channels, self.eps, self.slope, self.fused = in_features, _channels(channels), float(eps), float(slope), bool(fused)
        w = torch.empty(in_features, channels).normal_(0.0, math.sqrt(2.0 / in_features), generator=generator)
        self.weight = torch.nn.Parameter(w)
        self.params = torch.nn.Parameter(init_params(channels))

    def named_views(self):
        return views(self.params, self.channels)

    def forward(self, sim, x):
        z = x @ self.weight.to(x.dtype)
        if self.fused:
            return _function().apply(z, self.params, sim, self.eps, self.slope)
        return eager(z, self.params, self.eps, self.slope).to(x.dtype)


class MLP(_module_base()):
    """The reference's MLP(num_channels, num_layers): `layers` DenseNormAct of `channels` each, the first over
    in_features.  forward(sim, x [n, in_features]) -> [n, channels] in x's dtype.  fused=False runs eager() on the same
    parameters, for tools/mlp_bench.py and the tests."""

    def __init__(self, in_features, channels=256, layers=3, fused=True, eps=DEFAULT_EPS, slope=DEFAULT_SLOPE, generator=None):
        import torch
        super().__init__()
        if isinstance(layers, bool) or not isinstance(layers, int) or layers < 1:
            raise ValueError(f"layers must be a positive integer, got {layers}")
        self.in_features, self.channels = in_features, _channels(channels)
        self.layers = torch.nn.ModuleList(DenseNormAct(in_features if i == 0 else channels, channels, eps, slope, fused, generator)
                                          for i in range(layers))

    @property
    def fused(self):
        return all(layer.fused for layer in self.layers)

    @fused.setter
    def fused(self, value):
        for layer in self.layers:
            layer.fused = bool(value)

    def forward(self, sim, x):
        for layer in self.layers:
            x = layer(sim, x)
        return x
