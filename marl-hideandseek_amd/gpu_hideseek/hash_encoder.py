"""The SimHash encoder: the reference's HashNet (scripts/jax_policy.py:170-218, the network make_policy selects with
use_hash=True) over packed policy-input rows, forward by one kernel and parameter gradient by a binned sum
(hs_hash_encode, hs_hash_encode_backward, csrc/hs_k_hash.h).

HashNet concatenates self, agents, boxes and ramps (the column order of a packed row, policy_inputs.TABLES), projects
the 296 columns onto 8 directions, takes the 8 sign bits as a bin number 0 .. 255, looks the bin up in a [256, 32] table
and LayerNorms the looked-up row: 32 channels per row, which feed the recurrent core directly.  include/hideseek.h
states the arithmetic, IEEE f32 in a fixed order:

    enc = hash_encoder.HashEncoder().cuda()                          # one flat float32 Parameter of 10624 elements
    sim.pack_policy_inputs(actor=actor_rows[t], critic=critic_rows[t])
    feats = enc(sim, actor_rows[t])                                  # [rows, 32], part of the autograd graph
    loss = head(feats) ...; loss.backward(); optimiser.step()        # the backward kernels hand grad_params to autograd

or without autograd, into a rollout buffer:

    sim.hash_encode(actor_rows[t], enc.params.detach(), features=feat_buf[t])

The hash is a step function and the reference puts stop_gradient on it: no gradient with respect to the projection or
the rows exists, and the projection's part of grad_params is +0.  eager() is the same composition in plain torch, for
readers, tools/hash_bench.py and the tests; a row whose projection lies within rounding of zero may land in another bin
there than in the kernel (tests/test_hash_encoder_host.py bounds how many such rows there are).
"""
import ctypes as C
import functools
import math

from ._request import _DTYPES, _above_zero, _dtype_arg, _module_base, _name, _outputs, _run, _shard_calls, _tensor, _wanted
from .policy_inputs import ROW

BITS, BINS, FEATURES = 8, 256, 32             # HS_HASH_BITS, HS_HASH_BINS, HS_HASH_FEATURES: the reference's hash_power and feature_dim
PARAMS = BITS * ROW + BINS * FEATURES + 2 * FEATURES      # HS_HASH_PARAMS: 10624
ROWS_PER_ROUND = 8        # HS_HASH_ROWS_PER_ROUND: the rows a workgroup takes per round, two per wave
MAX_GRID_BWD = 256        # HS_HASH_MAX_GRID_BWD: workgroups (and workspace slices) of a backward call at the most
SUM_SEGS = 8              # HS_HASH_SUM_SEGS (= HS_EMBED_SUM_SEGS)
DEFAULT_EPS = 1e-6        # flax's LayerNorm epsilon


class HsHashEncodeRequest(C.Structure):
    """hs_hash_encode_request (include/hideseek.h)."""
    _fields_ = [("rows", C.c_void_p), ("params", C.c_void_p), ("n", C.c_int32), ("rows_dtype", C.c_int32), ("features_dtype", C.c_int32),
                ("eps", C.c_float), ("features", C.c_void_p), ("bin", C.c_void_p)]


class HsHashEncodeBackwardRequest(C.Structure):
    """hs_hash_encode_backward_request (include/hideseek.h)."""
    _fields_ = [("bin", C.c_void_p), ("grad_features", C.c_void_p), ("params", C.c_void_p), ("n", C.c_int32), ("grad_dtype", C.c_int32),
                ("eps", C.c_float), ("reserved", C.c_int32), ("grad_params", C.c_void_p)]


# ---- the parameters ----
def param_layout():
    """{part: (first, one past the last, shape)}: the element ranges of the flat parameter tensor of PARAMS float32, in
    order: the projection proj [8, 296] (direction major), the table [256, 32], and the LayerNorm's scale (gamma) and
    shift (beta)."""
    out, at = {}, 0
    for part, sh in (("proj", (BITS, ROW)), ("table", (BINS, FEATURES)), ("scale", (FEATURES,)), ("shift", (FEATURES,))):
        size = math.prod(sh)
        out[part] = (at, at + size, sh)
        at += size
    assert at == PARAMS
    return out


def views(params):
    """The named zero-copy views of a flat parameter (or gradient) tensor: {part: tensor} after param_layout."""
    if params.dim() != 1 or params.numel() != PARAMS:
        raise ValueError(f"params must have shape ({PARAMS},), got {tuple(params.shape)}")
    return {p: params[lo:hi].view(sh) for p, (lo, hi, sh) in param_layout().items()}


def init_params(generator=None):
    """A fresh flat float32 parameter tensor (on the CPU): proj standard normal (HashNet's random.normal), the table
    normal with standard deviation sqrt(2 / 256), scale 1 and shift 0.  The table's and the LayerNorm's initialisers are
    the project's choices: HashNet names jax's he_normal, whose fan convention the reference's tree does not pin for an
    embedding table, and its LayerNorm comes from madrona_learn, which is not part of that tree."""
    import torch
    p = torch.zeros(PARAMS, dtype=torch.float32)
    v = views(p)
    v["proj"].normal_(0.0, 1.0, generator=generator)
    v["table"].normal_(0.0, math.sqrt(2.0 / BINS), generator=generator)
    v["scale"].fill_(1.0)
    return p


def eager_bins(rows, params):
    """The bin [n] int64 of every row in plain torch, in the dtype of params."""
    import torch
    y = rows.to(params.dtype) @ views(params)["proj"].t()
    return ((y > 0).to(torch.int64) << torch.arange(BITS, device=y.device)).sum(-1)


def eager(rows, params, eps=DEFAULT_EPS):
    """The plain-torch composition in the dtype of params (float32, or float64 for a reference): [n, 32] features of rows
    [n, 296].  Differentiable in the table, the scale and the shift; the projection gets no gradient."""
    import torch
    v = views(params)
    with torch.no_grad():
        bins = eager_bins(rows, params)
    return torch.nn.functional.layer_norm(v["table"][bins], (FEATURES,), v["scale"], v["shift"], eps)


# ---- the fused calls ----
def request(gpu_id, rows, params, eps=DEFAULT_EPS, features=True, bin=None, dtype=None):
    """Validate a forward call over the n = rows.shape[0] rows on GPU `gpu_id`, allocate the outputs given as True
    (features in `dtype`, by default the dtype of the rows; bin uint8 [n]), and return ({name: tensor},
    HsHashEncodeRequest).  Raises ValueError before the library is involved."""
    import torch
    dev = torch.device("cuda", gpu_id)
    eps = _above_zero("eps", eps)
    _tensor("rows", rows, ("n >= 1", ROW), _DTYPES, dev, bound=ROW, align=16)
    _tensor("params", params, (PARAMS,), ("float32",), dev)
    n = int(rows.shape[0])
    if features is None or features is False:
        raise ValueError("features is not optional: True or a torch tensor")
    outputs = _wanted((("features", features), ("bin", bin)), "no features requested")
    _dtype_arg("dtype", dtype)
    specs = {"features": ((n, FEATURES), rows.dtype if dtype is None else dtype, _DTYPES), "bin": ((n,), torch.uint8)}
    res, ptr = _outputs(outputs, specs, [("rows", rows), ("params", params)], dev)
    req = HsHashEncodeRequest(rows.data_ptr(), params.data_ptr(), n, _DTYPES[_name(rows.dtype)], _DTYPES[_name(res["features"].dtype)], eps,
                              ptr("features"), ptr("bin"))
    return res, req


def request_backward(gpu_id, bin, grad_features, params, eps=DEFAULT_EPS, grad_params=True):
    """Validate a backward call, allocate grad_params when it is True, and return ({"grad_params": tensor},
    HsHashEncodeBackwardRequest).  Raises ValueError before the library is involved."""
    import torch
    dev = torch.device("cuda", gpu_id)
    eps = _above_zero("eps", eps)
    if not isinstance(bin, torch.Tensor) or not isinstance(grad_features, torch.Tensor):
        raise ValueError("bin and grad_features must be torch tensors")
    _tensor("bin", bin, ("n >= 1",), ("uint8",), dev, bound=ROW)
    n = int(bin.shape[0])
    _tensor("grad_features", grad_features, (n, FEATURES), _DTYPES, dev)
    _tensor("params", params, (PARAMS,), ("float32",), dev)
    inputs = [("bin", bin), ("grad_features", grad_features), ("params", params)]
    flat = ((PARAMS,), torch.float32, lambda k, t: _tensor(k, t, (PARAMS,), ("float32",), dev))      # the one output: not optional
    res, ptr = _outputs({"grad_params": grad_params}, {"grad_params": flat}, inputs, dev)
    req = HsHashEncodeBackwardRequest(bin.data_ptr(), grad_features.data_ptr(), params.data_ptr(), n, _DTYPES[_name(grad_features.dtype)], eps, 0,
                                      ptr("grad_params"))
    return res, req


def compute(sim, rows, params, stream=None, **kw):
    """HideAndSeekSimulator.hash_encode."""
    res, req = request(sim.gpu_id, rows, params, **kw)
    _run(sim, "hs_hash_encode", req, stream)
    return res


def compute_backward(sim, bin, grad_features, params, stream=None, **kw):
    """HideAndSeekSimulator.hash_encode_backward."""
    res, req = request_backward(sim.gpu_id, bin, grad_features, params, **kw)
    _run(sim, "hs_hash_encode_backward", req, stream)
    return res


def compute_sharded(ssim, rows, params, stream=None, features=True, bin=None, **kw):
    """ShardedSimulator.hash_encode: every shard encodes its own rows on its own device."""
    return _shard_calls(ssim, "hs_hash_encode", request, stream, dict(rows=rows), dict(params=params), dict(features=features, bin=bin), kw)


def compute_backward_sharded(ssim, bin, grad_features, params, stream=None, grad_params=True, **kw):
    """ShardedSimulator.hash_encode_backward: as compute_sharded; every shard's grad_params holds the sum over its own
    rows (add them for shared parameters)."""
    return _shard_calls(ssim, "hs_hash_encode_backward", request_backward, stream, dict(bin=bin, grad_features=grad_features),
                        dict(params=params), dict(grad_params=grad_params), kw)


# ---- the autograd face ----
@functools.lru_cache(maxsize=None)
def _function():
    import torch

    class _Encode(torch.autograd.Function):
        @staticmethod
        def forward(ctx, params, sim, rows, eps, dtype):
            out = compute(sim, rows, params.detach(), eps=eps, features=True, bin=True, dtype=dtype)
            ctx.save_for_backward(params, out["bin"])
            ctx.call = (sim, eps)
            return out["features"]

        @staticmethod
        def backward(ctx, grad):
            params, bins = ctx.saved_tensors
            sim, eps = ctx.call
            g = compute_backward(sim, bins, grad.contiguous(), params.detach(), eps=eps)["grad_params"]
            return g, None, None, None, None
    return _Encode


class HashEncoder(_module_base()):
    """The encoder as a torch module: one flat float32 Parameter `params` of PARAMS = 10624 elements (param_layout;
    named_views() gives proj, table, scale and shift as views).  forward(sim, rows) runs the forward kernel on `sim`'s
    device and returns features [n, 32] (in `dtype`, by default the rows' dtype) as part of the autograd graph of
    `params`: its backward runs the backward kernels.  rows get no gradient.

    The projection is deliberately part of the Parameter, with a gradient that is always +0: that way it travels with
    the flat buffer wherever the parameters go (optim.flatten, checkpoints, Population.apply_exploit, the past pool's
    copies, the sharded trainer's replicas and its gradient reduction), where a registered buffer would be left behind.
    Under Adam a parameter whose gradient is always zero never moves (its moments stay zero, so its step is 0 / eps), so
    the projection stays what init_params drew.  Weight decay, if it were ever set, would shrink it all the same."""

    def __init__(self, eps=DEFAULT_EPS, generator=None):
        import torch
        super().__init__()
        self.eps = float(eps)
        self.params = torch.nn.Parameter(init_params(generator))

    def named_views(self):
        return views(self.params)

    def forward(self, sim, rows, dtype=None):
        return _function().apply(self.params, sim, rows.detach(), self.eps, dtype)
