"""What the learner modules share on the way to a request entry point of libhideseek (include/hideseek.h): the dtype
codes, the checks of scalars and of tensors handed in, the plan of the outputs, and the two ways of calling — one handle,
blocking or on a stream, and one request per shard on side streams.  Internal: imported by the package's public modules.

Every request() checks in this order: the scalars, then shape, dtype and strides of every tensor (_tensor, _rows), then
that no output overlaps anything else, and the device last (_disjoint), so that every other fault is reported whatever
device the tensors are on.

Every *_sharded face follows _shard_calls: an input has one tensor per shard, on the shard's device; the parameters are
one tensor for every shard (which then all have to be on its device) or a list; an optional input, an output and
`stream` are True / None for all shards or a list with one entry per shard; the result is the list of the shards'
results.  With stream=None every shard's call is enqueued on a side stream of its device, ordered after that device's
current stream, before any is waited for."""
import ctypes as C
import math

_DTYPES = {"float32": 1, "bfloat16": 3, "float16": 4}      # HS_DTYPE_F32 / _BF16 / _F16
_names = {}                                                # dtype -> name, as _name found it


def _name(dtype):
    """"float32" of torch.float32 (kept: a request asks for a handful of names, each several times)."""
    try:
        return _names[dtype]
    except KeyError:
        return _names.setdefault(dtype, str(dtype).replace("torch.", ""))
    except TypeError:           # not hashable: no dtype, and the caller says so
        return str(dtype).replace("torch.", "")


def stream_handle(stream):
    """The raw hipStream_t of a torch.cuda.Stream (or the integer itself)."""
    return int(getattr(stream, "cuda_stream", stream))


def _module_base():
    """torch.nn.Module, for the class statements of the modules that keep torch out of their import lines."""
    import torch
    return torch.nn.Module


# ---- scalars ----
def _finite(name, x):
    """float(x), finite as a float and as the float32 a request carries."""
    v = float(x)
    if not math.isfinite(v) or not math.isfinite(C.c_float(v).value):
        raise ValueError(f"{name} must be finite, got {x}")
    return v


def _above_zero(name, x):
    """_finite, and above 0 after the rounding to float32."""
    v = _finite(name, x)
    if not C.c_float(v).value > 0.0:
        raise ValueError(f"{name} must be above 0, got {x}")
    return v


def _dtype_arg(name, dtype):
    """A dtype argument for an allocated output: None or one of _DTYPES."""
    if dtype is not None and _name(dtype) not in _DTYPES:
        raise ValueError(f"{name} must be one of {', '.join(_DTYPES)}, got {dtype}")


def _one_of(name, v, allowed):
    """An integer (no bool, no float) out of the tuple `allowed`."""
    if isinstance(v, bool) or not isinstance(v, int) or v not in allowed:
        raise ValueError(f"{name} must be one of {allowed}, got {v}")
    return v


# ---- tensors handed in ----
def _stride(t, L):
    """The row stride a request carries for a [n, W >= L] tensor that passed _rows."""
    return max(int(t.stride(0)) if t.shape[0] > 1 else int(t.shape[1]), L)


def _rows(name, t, n, L, dev, what):
    """Check a [n, W >= L] tensor that is contiguous in its last dimension (logits, grad_logits)."""
    import torch
    if not isinstance(t, torch.Tensor):
        raise ValueError(f"{name} must be a torch tensor")
    what = f"{name} must be a {' / '.join(_DTYPES)} tensor of shape ({what}, W >= {L}), contiguous in its last dimension, on {dev}"
    if t.dim() != 2 or t.shape[0] < 1 or (n is not None and t.shape[0] != n) or t.shape[1] < L:
        raise ValueError(f"{what}: its shape is {tuple(t.shape)}")
    if _name(t.dtype) not in _DTYPES:
        raise ValueError(f"{what}: its dtype is {t.dtype}")
    stride = _stride(t, L)
    if t.stride(1) != 1 or (t.shape[0] > 1 and t.stride(0) < L) or t.shape[0] * stride >= 2 ** 31:
        raise ValueError(f"{what}: its stride is {tuple(t.stride())} (n * stride must stay below 2^31)")
    return stride


def _shape_text(shape):
    return "(" + ", ".join(str(d) for d in shape) + ("," if len(shape) == 1 else "") + ")"


def _fits(got, shape):
    if got == shape:
        return True
    if len(got) != len(shape):
        return False
    for g, d in zip(got, shape):
        if g != d and not (isinstance(d, str) and g >= 1):
            return False
    return True


_OUTPUT = "True, None or a torch tensor"      # what an argument that names an output may be


def _tensor(name, t, shapes, dtypes, dev, kind="a torch tensor", bound=None, align=None):
    """The one check of a contiguous tensor handed in.  `shapes` is the accepted shape, or a list of alternatives; a
    dimension given as a string ("n >= 1", "T") is free and at least 1, and the string is how the message names it.
    `dtypes` are the accepted dtype names, `kind` is what a non-tensor is told `name` must be.  With `bound`, the leading
    dimension times `bound` must stay below 2^31 (the kernels index in int32); with `align`, the address must be a
    multiple of that many bytes.  The device is not looked at: _disjoint does that last, once every shape, dtype and
    stride has been reported.  The message is only put together when a check fails."""
    import torch
    if not isinstance(t, torch.Tensor):
        raise ValueError(f"{name} must be {kind}")
    got = t.shape
    if type(shapes) is not list:
        fit = _fits(got, shapes)
    else:
        fit = False
        for s in shapes:
            if _fits(got, s):
                fit = True
                break
    if not fit:
        fault = f"its shape is {tuple(got)}"
    elif _name(t.dtype) not in dtypes:
        fault = f"its dtype is {t.dtype}"
    elif not t.is_contiguous():
        fault = "it is not contiguous"
    elif bound is not None and got[0] * bound >= 2 ** 31:
        fault = f"n * {bound} must stay below 2^31"
    elif align is not None and t.data_ptr() % align:
        raise ValueError(f"{name} must be {align}-byte aligned: its address is {t.data_ptr():#x}")
    else:
        return
    alts = shapes if type(shapes) is list else [shapes]
    raise ValueError(f"{name} must be a contiguous {' / '.join(dtypes)} tensor of shape {' or '.join(map(_shape_text, alts))} on {dev}: {fault}")


def _vector(name, t, n, dev, dtypes, kind="a torch tensor"):
    """Check a contiguous per-sample tensor [n] or [n, 1]."""
    _tensor(name, t, [(n,), (n, 1)], dtypes, dev, kind)


LOSS_SCALE_STATE = 4      # HS_LOSS_SCALE_STATE: S, good steps since S last changed, backoffs, growths


def _loss_scale_input(loss_scale, dev):
    """[("loss_scale", tensor)] for the inputs of a request, or [] without one: the state of optim.LossScale, float64
    [LOSS_SCALE_STATE], contiguous (8-byte aligned with that)."""
    if loss_scale is None:
        return []
    _tensor("loss_scale", loss_scale, (LOSS_SCALE_STATE,), ("float64",), dev, "None or a torch tensor", align=8)
    return [("loss_scale", loss_scale)]


def _overlap(a, b):
    """Whether the storage ranges of two tensors intersect."""
    def span(t):
        last = sum((s - 1) * st for s, st in zip(t.shape, t.stride()))
        return t.data_ptr(), t.data_ptr() + (last + 1) * t.element_size()
    (a0, a1), (b0, b1) = span(a), span(b)
    return a0 < b1 and b0 < a1


def _disjoint(outputs, inputs, dev):
    """No output [(name, tensor)] overlaps an input or an earlier output, and then all of them are on `dev`: shapes,
    dtypes and strides have been checked first, so that every one of them is reported whatever device the tensors are on."""
    for k, t in outputs:
        for k2, t2 in inputs:
            if _overlap(t, t2):
                raise ValueError(f"{k} overlaps {k2}")
    for i, (k, t) in enumerate(outputs):
        for k2, t2 in outputs[:i]:
            if _overlap(t, t2):
                raise ValueError(f"{k} overlaps {k2}")
    for k, t in inputs + outputs:
        if t.device != dev:
            raise ValueError(f"{k} must be on {dev}: it is on {t.device}")


# ---- the outputs of a request ----
def _wanted(pairs, nothing):
    """{name: argument} of the outputs [(name, argument)] that are asked for (True or a tensor; None and False are not),
    in the order given; none at all raises "nothing to do: `nothing`"."""
    outputs = {k: t for k, t in pairs if t is not None and t is not False}
    if not outputs:
        raise ValueError(f"nothing to do: {nothing}")
    return outputs


def _outputs(wanted, specs, inputs, dev):
    """The outputs of a request: `wanted` as _wanted returned it, `inputs` [(name, tensor)], and `specs` {name: (shape,
    dtype[, accepted or check[, zeros]])}: an output given as True is allocated as torch.empty (torch.zeros with `zeros`)
    of `shape` and `dtype`; one given as a tensor is checked by check(name, tensor) where the third entry is callable,
    else by _tensor with that shape and the `accepted` dtype names (by default `dtype` alone).  Checks every tensor given,
    then that none overlaps an input or another, then that everything is on `dev` (_disjoint), and allocates last.
    Returns ({name: tensor} in the order of `wanted`, ptr), where ptr(name) is the address of an output, or None for one
    not asked for."""
    import torch
    given = [(k, t) for k, t in wanted.items() if t is not True]
    for k, t in given:
        spec = specs[k]
        third = spec[2] if len(spec) > 2 else None
        if callable(third):
            third(k, t)
        else:
            _tensor(k, t, spec[0], third or (_name(spec[1]),), dev, _OUTPUT)
    _disjoint(given, inputs, dev)
    res = {}
    for k, t in wanted.items():
        if t is True:
            spec = specs[k]
            t = (torch.zeros if len(spec) > 3 and spec[3] else torch.empty)(spec[0], dtype=spec[1], device=dev)
        res[k] = t
    return res, lambda k: res[k].data_ptr() if k in res else None


# ---- one entry per shard ----
def _per_shard(ssim, name, arg):
    import torch
    n = len(ssim.shards)
    if arg is None or arg is True or arg is False:
        return [arg] * n
    if isinstance(arg, torch.Tensor) or len(arg) != n:
        raise ValueError(f"{name}: one entry per shard ({n}) expected")
    return list(arg)


# ---- the calls ----
_enqueue = [0]              # depth of on_current_stream() contexts


class on_current_stream:
    """Inside this context a call given stream=None is enqueued on torch's current stream of the handle's device without
    waiting, where it would otherwise block: the module faces (EntityEncoder, MLP, LSTMCore and their backward) pass no
    stream, and the update loop (gpu_hideseek.trainer) runs them here so that nothing in it waits for the device."""

    def __enter__(self):
        _enqueue[0] += 1
        return self

    def __exit__(self, *exc):
        _enqueue[0] -= 1
        return False


def _run(sim, fn, req, stream, *extra):
    """Entry point `fn` of `sim`'s handle with request `req` (and what follows it in the signature): blocking with
    stream=None (outside on_current_stream()), else `fn`_async on the torch.cuda.Stream or raw handle, without
    synchronising."""
    from ._native import check
    if stream is None and _enqueue[0]:
        import torch
        stream = torch.cuda.current_stream(sim.gpu_id)
    if stream is None:
        check(getattr(sim._L, fn)(sim._h, C.byref(req), *extra))
    else:
        check(getattr(sim._L, fn + "_async")(sim._h, C.c_void_p(stream_handle(stream)), C.byref(req), *extra))


def _sharded(ssim, fn, make, stream):
    """make(i, shard) -> (result, request) for every shard, then entry point `fn` (a name for _run, or a callable
    (shard, request, stream)) for each on the shard's entry of `stream`; with None there, on a side stream of its device
    ordered after that device's current stream, all of which are waited for once every call is enqueued.  Returns the
    list of the shards' results."""
    import torch
    streams = _per_shard(ssim, "stream", stream)
    reqs = [make(i, s) for i, s in enumerate(ssim.shards)]
    waits = []
    for s, (res, req), st in zip(ssim.shards, reqs, streams):
        if st is None:
            st = torch.cuda.Stream(device=s.gpu_id)
            st.wait_stream(torch.cuda.current_stream(s.gpu_id))
            waits.append(st)
        if callable(fn):
            fn(s, req, st)
        else:
            _run(s, fn, req, st)
    for st in waits:
        st.synchronize()
    return [res for res, _ in reqs]


def _shard_calls(ssim, fn, request, stream, required, shared=None, per_shard=None, kw=None, lead=lambda s: (s.gpu_id,)):
    """The *_sharded face of a module: request(*lead(shard), **arguments of the shard, **kw) for every shard, run by
    _sharded.  `required` {name: list} are the inputs with one tensor per shard, `shared` {name: tensor or list} the
    parameters (one tensor is handed to every shard), `per_shard` {name: True / None / list} the optional inputs and
    the outputs; `kw` goes to every shard as it is.  The module docstring states the conventions."""
    import torch
    n = len(ssim.shards)
    args = {}
    for k, arg in required.items():
        if isinstance(arg, torch.Tensor) or arg is None or len(arg) != n:
            raise ValueError(f"{k}: one tensor per shard ({n}) expected")
        args[k] = arg
    for k, arg in (shared or {}).items():
        args[k] = [arg] * n if isinstance(arg, torch.Tensor) else _per_shard(ssim, k, arg)
    for k, arg in (per_shard or {}).items():
        args[k] = _per_shard(ssim, k, arg)
    return _sharded(ssim, fn, lambda i, s: request(*lead(s), **{k: v[i] for k, v in args.items()}, **(kw or {})), stream)
