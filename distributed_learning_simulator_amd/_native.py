"""ctypes binding of libdls_hip.so (the C-ABI declared in include/dls_hip.h).

Every wrapper takes torch tensors that already live on the current HIP device,
passes raw pointers and the current stream to the library, and raises
``RuntimeError`` (with ``dls_last_error()``) on a non-zero status.  There is no
CPU or PyTorch fallback: if the library cannot be loaded, or a tensor is not on
the GPU, the call fails loudly.
"""
import ctypes
import math
import os
import threading

import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("DLS_HIP_LIB", os.path.join(_HERE, "libdls_hip.so"))

FEDAVG_EXACT = 0
FEDAVG_FMA = 1
SIGN_NAN_MARK = 1 << 24
QTILE_GROUPS = 10  # DLS_QTILE_GROUPS
SUBSET_UNION_MAX = 64  # DLS_SUBSET_UNION_MAX: coalitions per dls_subset_fedavg_union_f32 call
ROBUST_MAX_K = 64  # DLS_ROBUST_MAX_K: client rows per dls_trimmed_mean_f32 call
SECAGG_MAX_STREAMS = 1088  # DLS_SECAGG_MAX_STREAMS: masks added and removed per secagg call


def sign_words(P):
    """uint64 words per client row of sign planes (DLS_SIGN_WORDS)."""
    return ((P + 255) // 256) * 8


def sign_row_pitch(P):
    """The row pitch (uint64 words) of a store of sign-plane rows: sign_words(P)
    rounded up to 128 bytes, so that every row starts on a cache line and the
    vote's 128-byte-aligned wave ranges never share a line (dls_sign_vote)."""
    return (sign_words(P) + 15) // 16 * 16


class QTile(ctypes.Structure):
    """struct dls_qtile (include/dls_hip.h)."""

    _fields_ = [
        ("dst", ctypes.c_int64),
        ("src", ctypes.c_int64),
        ("len", ctypes.c_int32),
        ("kind", ctypes.c_int32),
        ("chan0", ctypes.c_int32),
        ("row_len", ctypes.c_int32),
        ("row_pos", ctypes.c_int32),
        ("chan_end", ctypes.c_int32),
    ]


_i32, _i64, _f32, _p, _u64 = (ctypes.c_int32, ctypes.c_int64, ctypes.c_float, ctypes.c_void_p,
                              ctypes.c_uint64)
_u32, _f64 = ctypes.c_uint32, ctypes.c_double

# name -> argtypes (restype int unless noted); mirrors include/dls_hip.h
SIGNATURES = {
    "dls_last_error": ([], ctypes.c_char_p),
    "dls_abi_version": ([], _i32),
    "dls_source_hash": ([], ctypes.c_char_p),
    "dls_device_count": ([], _i32),
    "dls_two_constant_division": ([_f32], _i32),
    "dls_fedavg_f32": ([_p, _i64, _p, _p, _i32, _f32, _i64, _i32, _p, _p], _i32),
    "dls_subset_fedavg_f32": ([_p, _i64, _p, _p, _p, _p, _i32, _i64, _p, _i64, _p], _i32),
    "dls_subset_fedavg_union_f32": ([_p, _i64, _p, _p, _p, _i32, _p, _i32, _i64, _p, _i64, _p],
                                    _i32),
    "dls_trimmed_mean_f32": ([_p, _i64, _p, _i32, _i32, _i64, _p, _p], _i32),
    "dls_mean_around_median_f32": ([_p, _i64, _p, _i32, _i32, _i64, _p, _p], _i32),
    "dls_craft_rows_f32": ([_p, _i64, _p, _i32, _p, _i32, _f32, _f32, _p, _i64, _p], _i32),
    "dls_pairwise_sqdist_workspace": ([_i32, _i64], _i64),
    "dls_pairwise_sqdist_f32": ([_p, _i64, _p, _i32, _i64, _p, _p, _p], _i32),
    "dls_rows_gram_workspace": ([_i32, _i64], _i64),
    "dls_rows_gram_f32": ([_p, _i64, _p, _i32, _i64, _p, _p, _p, _p], _i32),
    "dls_history_gram_f32": ([_p, _i64, _p, _p, _i64, _p, _i32, _i64, _p, _p, _p, _p], _i32),
    "dls_weiszfeld_workspace": ([_i32, _i64], _i64),
    "dls_rows_sqdist_to_f32": ([_p, _i64, _p, _i32, _i64, _p, _p, _p, _p], _i32),
    "dls_weiszfeld_step_f32": ([_p, _i64, _p, _i32, _p, _i64, _p, _p, _p, _p], _i32),
    "dls_centered_clip_step_f32": ([_p, _i64, _p, _i32, _p, _i64, _p, _p, _p, _p], _i32),
    "dls_server_opt_step_f32": ([_i32, _p, _p, _p, _p, _p, _i64, _f32, _f32, _f32, _f32, _f32, _f32,
                                 _p], _i32),
    "dls_topk_workspace": ([_i64], _i64),
    "dls_topk_compress_f32": ([_p, _p, _p, _i64, _i64, _p, _p, _p, _p, _p], _i32),
    "dls_sparse_fedavg_f32": ([_p, _p, _p, _p, _p, _i32, _f32, _i64, _p, _p], _i32),
    "dls_philox_u32": ([_p, _i64, _u64, _u64, _i64, _p], _i32),
    "dls_philox_normal_f32": ([_p, _i64, _u64, _u64, _i64, _p], _i32),
    "dls_normal_from_bits_f32": ([_p, _i64, _p, _p], _i32),
    "dls_dp_clip_noise_step_f32": ([_p, _i64, _p, _i32, _p, _i64, _p, _f32, _u64, _u64, _p],
                                   _i32),
    "dls_secagg_mask_f32": ([_p, _p, _i64, _i32, _i32, _u32, _p, _i32, _p, _i32, _u64, _p, _p, _p],
                            _i32),
    "dls_secagg_unmask_f32": ([_p, _i64, _p, _i32, _p, _i32, _p, _i32, _u64, _p, _i32, _f64, _i64,
                               _p, _p, _p], _i32),
    "dls_subset_gemm_f32": ([_p, _i32, _i32, _p, _i64, _p, _i64, _p, _i64, _p], _i32),
    "dls_sign_pack_f32": ([_p, _i64, _i32, _i64, _p, _i64, _p, _p], _i32),
    "dls_sign_vote_count": ([_p, _i64, _p, _i32, _i64, _p, _p], _i32),
    "dls_sign_from_counts": ([_p, _i64, _p, _p, _p], _i32),
    "dls_sign_vote": ([_p, _i64, _p, _i32, _i64, _p, _p, _p, _p], _i32),
    "dls_sign_vote_geometry": ([_i64, _i32, _i32, _p, _p, _p], _i32),
    "dls_sign_vote_wave_ranges": ([_i64, _i32, _i32, _i64, _i64, _p, _p], _i32),
    "dls_sign_sgd_direction": ([_p, _p, _i64, _f32, _f32, _i32, _i32, _p, _p, _p], _i32),
    "dls_sign_sgd_apply": ([_p, _p, _i64, _f32, _f32, _p], _i32),
    "dls_dequant_fedavg": ([_p, _i32, _p, _p, _i64, _p, _i64, _p, _i64, _i64, _p, _p, _i32, _f32,
                            _p, _p],
                           _i32),
    "dls_dequant_fedavg_mode": ([_p, _i32, _p, _p, _i64, _p, _i64, _p, _i64, _i64, _p, _p, _i32,
                                 _f32, _i32, _p, _p], _i32),
    "dls_segment_minmax_f32": ([_p, _p, _i32, _p, _p, _i64, _p], _i32),
    "dls_qparams_minmax": ([_p, _p, _i32, _i32, _i32, _i32, _p, _p, _p], _i32),
    "dls_quantize_affine": ([_p, _p, _i32, _p, _p, _i32, _i32, _p, _p, _i32, _u64, _i64, _p],
                            _i32),
    "dls_bn_fold_f32": ([_p, _p, _p, _p, _f32, _i32, _p, _p, _p], _i32),
    "dls_bn_act_nhwc_f32": ([_p, _i64, _i32, _p, _p, _p, _i32, _p, _p], _i32),
    "dls_bn_fold_exact_f32": ([_p, _p, _p, _p, _f32, _i32, _p, _p], _i32),
    "dls_bn_act_exact_nhwc_f32": ([_p, _i64, _i32, _p, _p, _i32, _p, _p], _i32),
    "dls_bn_act_exact_nchw_f32": ([_p, _i64, _i32, _i64, _p, _p, _i32, _p, _p], _i32),
    "dls_conv_pack_input_f32": ([_p, _i64, _i32, _i32, _i32, _i32, _p, _p], _i32),
    "dls_conv_pack_weights_f32": ([_p, _i32, _i32, _i32, _i32, _i32, _p, _p], _i32),
    "dls_conv_pack_im2col_f32": ([_p, _i64, _i32, _i32, _i32, _i32, _i32, _i32, _i32, _i32, _p, _p],
                                 _i32),
    "dls_conv_pack_weights_im2col_f32": ([_p, _i32, _i32, _i32, _i32, _i32, _p, _p], _i32),
    "dls_conv_bn_act_split": ([_p, _i64, _i32, _i32, _i32, _p, _i32, _i32, _i32, _i32, _i32, _p, _p,
                               _i32, _p, _p], _i32),
    "dls_conv_stem_bn_act_f32": ([_p, _i64, _i32, _i32, _i32, _p, _i32, _i32, _i32, _i32, _i32, _p,
                                  _i32, _p, _p], _i32),
    "dls_pool_linear_split": ([_p, _i64, _i32, _i32, _p, _p, _i32, _p, _p], _i32),
    "dls_conv_kernel_choice": ([_i64, _i32, _i32, _i32, _i32, _i32, _i32, _i32, _i32], _i32),
    "dls_conv_stem_kernel_choice": ([_i64, _i32, _i32, _i32, _i32, _i32, _i32, _i32, _i32], _i32),
    "dls_lenet5_eval_f32": ([_p, _i64, _i32, _p, _p, _i64, _p, _i32, _p, _p, _p], _i32),
    "dls_lenet5_eval_loss_f32": ([_p, _i64, _i32, _p, _p, _i64, _p, _i32, _p, _p, _p, _i64, _p],
                                 _i32),
    "dls_softmax_ce_f32": ([_p, _i32, _i64, _i32, _p, _p, _i64, _p], _i32),
    "dls_sum_rows_f64": ([_p, _i64, _i32, _i64, _p, _p], _i32),
}

_lib = None
_lock = threading.Lock()


def lib():
    """Load libdls_hip.so once (raises if it was not built)."""
    global _lib
    if _lib is None:
        with _lock:
            if _lib is None:
                if not os.path.exists(LIB_PATH):
                    raise RuntimeError(
                        f"libdls_hip.so not found at {LIB_PATH}; build it with "
                        "`make -C distributed_learning_simulator_amd/csrc` (no CPU fallback)")
                L = ctypes.CDLL(LIB_PATH)
                for name, (args, res) in SIGNATURES.items():
                    f = getattr(L, name)
                    f.argtypes = args
                    f.restype = res
                _lib = L
    return _lib


def _check(rc, name):
    if rc != 0:
        msg = lib().dls_last_error().decode(errors="replace")
        raise RuntimeError(f"{name} failed (status {rc}): {msg}")


def _ptr(t):
    if t is None:
        return None
    if not t.is_cuda:
        raise RuntimeError("libdls_hip: tensor is not on the GPU (no CPU fallback)")
    return ctypes.c_void_p(t.data_ptr())


def _stream(stream=None, like=None):
    """The given stream, else the current stream of `like`'s device (worker threads
    may run with another current device than the tensors they launch on)."""
    if stream is None:
        dev = like.device if like is not None and like.is_cuda else None
        stream = torch.cuda.current_stream(dev)
    return ctypes.c_void_p(stream.cuda_stream)


CSRC_HASHED = [  # the Makefile's HASHED, in its order
    "dls_runtime.hip",
    "fedavg.hip",
    "sign.hip",
    "quant.hip",
    "quant_fma.hip",
    "shapley.hip",
    "infer.hip",
    "conv.hip",
    "lenet.hip",
    "loss.hip",
    "robust.hip",
    "pairdist.hip",
    "weiszfeld.hip",
    "gram.hip",
    "serveropt.hip",
    "secagg.hip",
    "topk.hip",
    "dpnoise.hip",
    "dls_common.h",
    "quant_common.h",
    "loss_common.h",
    "sign_geometry.h",
    "rows_common.h",
    "philox_common.h",
    os.path.join("..", "..", "include", "dls_hip.h"),
]


def source_hash():
    """SHA-256 prefix of the library sources in this tree (the Makefile's
    dls_source_hash recipe); compare with lib().dls_source_hash()."""
    import hashlib
    h = hashlib.sha256()
    for f in CSRC_HASHED:
        with open(os.path.join(_HERE, "csrc", f), "rb") as fh:
            h.update(fh.read())
    return h.hexdigest()[:16]


def two_constant_division(divisor):
    """1 if the dequant kernels divide by fl32(divisor) with the two-constant method
    (proven correctly rounded for it by the library's exhaustive host check)."""
    return int(lib().dls_two_constant_division(float(divisor)))


def require_gpu():
    if not torch.cuda.is_available():
        raise RuntimeError("distributed_learning_simulator_amd needs a ROCm GPU (no CPU fallback)")
    lib()


# ---------------------------------------------------------------------- FedAvg
def fedavg(U, rows, weight, total, P, out, mode=FEDAVG_EXACT, stream=None):
    """servers/fed_server.py:44-66 over rows of U (see dls_fedavg_f32)."""
    assert U.dtype == torch.float32 and out.dtype == torch.float32
    assert rows.dtype == torch.int32 and weight.dtype == torch.float32
    _check(lib().dls_fedavg_f32(_ptr(U), U.stride(0), _ptr(rows), _ptr(weight), rows.numel(),
                                float(total), P, mode, _ptr(out), _stream(stream, U)),
           "dls_fedavg_f32")
    return out


# ------------------------------------------------- the operand checks, one of each
# The rows family (trimmed mean .. centered clip) and the vector calls after it state
# their operand contract with these; the library checks it again (csrc/rows_common.h).
_DTYPE_NAMES = {torch.float32: "fp32", torch.float64: "fp64", torch.int32: "int32",
                torch.int64: "int64"}


def _check_tensor(fn, name, t, dtype, n, what, exact=True, contiguous=True, device=None):
    """The one tensor check: ``t`` holds ``dtype`` (on ``device``, if given) and n, a
    shape tuple: has exactly that shape, contiguous; an int with ``contiguous``: exactly
    n elements of any shape, contiguous; an int without: is 1-D with unit stride and at
    least (``exact``: exactly) n elements.  ``what`` ends the message (a string, or a
    function that makes it: it is only wanted on failure)."""
    ok = torch.is_tensor(t) and t.dtype == dtype and (device is None or t.device == device)
    if ok and isinstance(n, tuple):
        ok = tuple(t.shape) == n and t.is_contiguous()
    elif ok and contiguous:
        ok = t.numel() == n and t.is_contiguous()
    elif ok:
        ok = (t.dim() == 1 and (t.numel() == n if exact else t.numel() >= n)
              and (t.numel() <= 1 or t.stride(0) == 1))
    if not ok:
        raise RuntimeError(f"{fn}: {name} must be {what() if callable(what) else what}")


def _unit_vector(fn, name, t, dtype, n, exact=False, count=None):
    """t: a ``dtype`` vector with unit stride of at least (``exact``: exactly) n elements
    (``count``: a (label, n) pair the message writes as label=n)."""
    _check_tensor(fn, name, t, dtype, n, lambda: f"an {_DTYPE_NAMES[dtype]} vector of "
                  f"{'exactly' if exact else 'at least'} {n if count is None else '%s=%s' % count} elements "
                  "with unit stride", exact=exact, contiguous=False)


def _f32_vector(fn, name, t, P):
    _unit_vector(fn, name, t, torch.float32, P, count=("P", P))


def _k_tensor(fn, name, t, dtype, shape):
    """t: a contiguous tensor of ``shape``, (K,) or (K, K), and ``dtype``."""
    _check_tensor(fn, name, t, dtype, shape, lambda: f"a contiguous {_DTYPE_NAMES[dtype]} "
                  f"[{', '.join('K' * len(shape))}] = {list(shape)} tensor")


def _f64_out(fn, name, t, shape):
    """An optional output (None: the wrapper allocates it): contiguous fp64 of ``shape``."""
    if t is not None:
        _k_tensor(fn, name, t, torch.float64, shape)


def _check_same_device(fn, x, /, _anchor="the input", **others):
    """Every given tensor (None: skipped) is on x's device; the message calls x ``_anchor``."""
    for name, t in others.items():
        if t is not None and t.device != x.device:
            raise RuntimeError(f"{fn}: {name} is on {t.device}, {_anchor} on {x.device}")


def _overlaps(a, b):
    """True if the storage ranges of a and b intersect."""
    a0 = a.data_ptr()
    b0 = b.data_ptr()
    return a0 < b0 + b.numel() * b.element_size() and b0 < a0 + a.numel() * a.element_size()


def _check_disjoint(tensors, message, allowed=None):
    """No two of the name -> tensor pairs overlap, but for a pair ``allowed(a, b)``
    exempts; ``message`` is formatted with the two names."""
    names = list(tensors)
    for i, a in enumerate(names):
        for b in names[i + 1:]:
            if not (allowed and allowed(a, b)) and _overlaps(tensors[a], tensors[b]):
                raise RuntimeError(message.format(a=a, b=b))


def _aligned16(fn, **tensors):
    """Every given tensor (None: skipped) starts on a 16-byte boundary; the message
    names all of them."""
    if any(t is not None and t.data_ptr() % 16 != 0 for t in tensors.values()):
        *head, last = tensors
        raise RuntimeError(f"{fn}: {', '.join(head) + ' and ' if head else ''}{last} must be "
                           "16-byte aligned")


def _row_pitch(t):
    """The element pitch of the rows of a matrix (one row: its width)."""
    return t.stride(0) if t.shape[0] > 1 else t.shape[1]


def _rows_operands(fn, U, rows, P, names=("U", "rows"), dtype=torch.float32):
    """The checks every rows-family wrapper makes on a matrix, a row table and P
    (``names``: what the messages call the two tensors; ``dtype``: the matrix's): returns
    (K, P, ldu)."""
    return (_rows_table(fn, U, rows, names, dtype),) + _rows_extent(fn, U, P)


def _rows_table(fn, U, rows, names=("U", "rows"), dtype=torch.float32):
    """The first half of ``_rows_operands``, the two tensors: returns K."""
    if (not torch.is_tensor(U) or U.dtype != dtype or U.dim() != 2
            or (U.shape[1] > 1 and U.stride(1) != 1)):
        raise RuntimeError(f"{fn}: {names[0]} must be an {_DTYPE_NAMES[dtype]} [rows, ld] matrix "
                           "with unit element stride")
    # 1-D with unit stride and any length (K is checked below) is "contiguous 1-D"
    _check_tensor(fn, names[1], rows, torch.int32, 0, "a contiguous int32 [K] tensor",
                  exact=False, contiguous=False)
    K = rows.numel()
    if not 1 <= K <= ROBUST_MAX_K:
        raise RuntimeError(f"{fn}: K={K} rows (1..ROBUST_MAX_K={ROBUST_MAX_K})")
    return K


def _rows_extent(fn, U, P):
    """The second half, P against the matrix (trimmed_mean checks its trim between the
    two): returns (P, ldu)."""
    P = int(P)
    if P < 0 or P % 4 != 0 or P > U.shape[1]:
        raise RuntimeError(f"{fn}: P={P} must be a multiple of 4 and at most the row "
                           f"length {U.shape[1]}")
    ldu = _row_pitch(U)
    if ldu % 4 != 0 or ldu < P:
        raise RuntimeError(f"{fn}: row pitch {ldu} must be a multiple of 4, at least P")
    return P, ldu


def _rows_placement(fn, U, aligned, **others):
    """The last two checks of a rows-family wrapper: the other operands on U's device, then
    U and the ``aligned`` ones among them on 16-byte boundaries."""
    _check_same_device(fn, U, **others)
    _aligned16(fn, U=U, **{name: others[name] for name in aligned})


def _workspace_call(entry, query, K, P, head, out, shape, stream):
    """The tail of the workspace-taking wrappers.  ``head``: the entry point's arguments
    before (fp64 result, workspace, stream), the matrix U first, tensors as they are;
    ``out``: the checked result or None (a new fp64 tensor of ``shape``).  Every operand
    goes through ``_ptr`` before the library is touched (no CPU path); the workspace is
    what ``query`` asks for, kept alive for a given ``stream``.  Returns out."""
    U = head[0]
    if out is None:
        out = torch.empty(shape, dtype=torch.float64, device=U.device)
    args = [_ptr(x) if torch.is_tensor(x) else x for x in head] + [_ptr(out)]
    nbytes = int(getattr(lib(), query)(K, P))
    if nbytes < 0:
        _check(nbytes, query)
    work = torch.empty(max(nbytes, 16), dtype=torch.uint8, device=U.device)
    _check(getattr(lib(), entry)(*args, _ptr(work), _stream(stream, U)), entry)
    if stream is not None:
        work.record_stream(stream)
    return out


def _to_one_row(fn, U, ldu, rows, K, param, P, out, stream):
    """The tail of trimmed_mean and mean_around_median: dls_<fn>_f32 with the rule's ``param``."""
    _f32_vector(fn, "out", out, P)
    _rows_placement(fn, U, ("out",), rows=rows, out=out)
    if P != 0:
        _check(getattr(lib(), f"dls_{fn}_f32")(_ptr(U), ldu, _ptr(rows), K, param, P, _ptr(out),
                                               _stream(stream, U)), f"dls_{fn}_f32")
    return out


def trimmed_mean(U, rows, trim, P, out, stream=None):
    """Coordinate-wise trimmed mean of the K = rows.numel() selected rows of U into
    out[:P] (dls_trimmed_mean_f32): per coordinate the ``trim`` lowest and highest
    values are dropped and the rest averaged in ascending order; trim = (K-1)//2 is
    the median.  The client weights play no part.  U: fp32 [*, ld] rows with unit
    element stride; rows: int32 [K], 1 <= K <= ROBUST_MAX_K; 0 <= 2*trim < K; P a
    multiple of 4, at most the row length."""
    fn = "trimmed_mean"
    K = _rows_table(fn, U, rows)
    trim = int(trim)
    if trim < 0 or 2 * trim >= K:
        raise RuntimeError(f"{fn}: trim={trim} (0 <= 2*trim < K={K})")
    P, ldu = _rows_extent(fn, U, P)
    return _to_one_row(fn, U, ldu, rows, K, trim, P, out, stream)


# DLS_PAIRDIST_MAX_WAVES (include/dls_hip.h): past it a wave takes several periods
PAIRDIST_MAX_WAVES = 2048


def pairwise_sqdist(U, rows, P, out=None, stream=None):
    """Squared Euclidean distances between the K = rows.numel() selected rows of U over
    their first P elements (dls_pairwise_sqdist_f32): an fp64 [K, K] device tensor,
    symmetric in bits with a +0.0 diagonal, each entry within 2^-17 relative of the
    exact squared distance of the fp32 rows; an entry of a row that holds inf or NaN
    is +inf or NaN.  U: fp32 [*, ld] rows with unit element stride; rows: int32 [K],
    1 <= K <= ROBUST_MAX_K; P a multiple of 4, at most the row length; out: a
    contiguous fp64 [K, K] tensor (default: a new one)."""
    fn = "pairwise_sqdist"
    K, P, ldu = _rows_operands(fn, U, rows, P)
    _f64_out(fn, "out", out, (K, K))
    _rows_placement(fn, U, (), rows=rows, out=out)
    return _workspace_call("dls_pairwise_sqdist_f32", "dls_pairwise_sqdist_workspace", K, P,
                           (U, ldu, rows, K, P), out, (K, K), stream)


def rows_gram(U, rows, P, base=None, out=None, stream=None):
    """Inner products of the K = rows.numel() selected rows of U over their first P
    elements (dls_rows_gram_f32): an fp64 [K, K] device tensor G[a][b] ~ sum_p h_a h_b,
    h_k = U[rows[k]] - base (one fp32 rounding) or the row itself without ``base``.
    Symmetric in bits; |G[a][b] - exact| <= 2^-17 * sum_p |h_a h_b|, so a cosine
    G[a][b] / sqrt(G[a][a] G[b][b]) is within 2^-17 absolute; rows of equal contents
    give G[a][b] == G[a][a] == G[b][b] bit for bit; a row that holds inf or NaN makes its
    own row and column non-finite.  U, rows, P as in pairwise_sqdist; base: None or an
    fp32 vector of at least P elements; out: a contiguous fp64 [K, K] tensor (default:
    a new one)."""
    fn = "rows_gram"
    K, P, ldu = _rows_operands(fn, U, rows, P)
    if base is not None:
        _f32_vector(fn, "base", base, P)
    _f64_out(fn, "out", out, (K, K))
    _rows_placement(fn, U, ("base",), rows=rows, base=base, out=out)
    return _workspace_call("dls_rows_gram_f32", "dls_rows_gram_workspace", K, P,
                           (U, ldu, rows, K, P, base), out, (K, K), stream)


def history_gram(U, rows, H, hrows, P, base=None, out=None, stream=None):
    """The fused FoolsGold step (dls_history_gram_f32): H[hrows[k]][:P] += U[rows[k]][:P]
    - base in place (the subtraction and the addition each rounded once to fp32, so
    numpy float32 reproduces the new H bit for bit; without ``base`` the row itself is
    added) and the Gram matrix of the new history rows, as ``rows_gram`` would give it,
    from the same visit: U, H and base are each read once and H is written once.
    Columns P.. of H and the rows not listed in ``hrows`` are untouched.  H: fp32
    [*, ldh] like U, not overlapping U or base; hrows: int32 [K] like rows.  The row
    tables are copied to the host once and checked: every index inside its matrix and
    ``hrows`` distinct (two lanes folding into one row would race).  Returns (H, G)."""
    fn = "history_gram"
    K, P, ldu = _rows_operands(fn, U, rows, P)
    Kh, _, ldh = _rows_operands(fn, H, hrows, P, names=("H", "hrows"))
    if Kh != K:
        raise RuntimeError(f"{fn}: hrows holds {Kh} rows, rows holds {K}")
    if base is not None:
        _f32_vector(fn, "base", base, P)
    _f64_out(fn, "out", out, (K, K))
    _rows_placement(fn, U, ("H", "base"), rows=rows, H=H, hrows=hrows, base=base, out=out)
    if _overlaps(H, U) or (base is not None and _overlaps(H, base)):
        raise RuntimeError(f"{fn}: H must not overlap U or base")
    _ptr(U), _ptr(rows), _ptr(H), _ptr(hrows), _ptr(base)  # no CPU path
    for name, table, n in (("rows", rows, U.shape[0]), ("hrows", hrows, H.shape[0])):
        idx = table.cpu().tolist()
        if min(idx) < 0 or max(idx) >= n:
            raise RuntimeError(f"{fn}: {name} {idx} outside the matrix's {n} rows")
        if name == "hrows" and len(set(idx)) != K:
            raise RuntimeError(f"{fn}: hrows must be distinct, not {idx}")
    return H, _workspace_call("dls_history_gram_f32", "dls_rows_gram_workspace", K, P,
                              (U, ldu, rows, H, ldh, hrows, K, P, base), out, (K, K), stream)


def mean_around_median(U, rows, keep, P, out, stream=None):
    """Coordinate-wise mean around the median of the K = rows.numel() selected rows of U
    into out[:P] (dls_mean_around_median_f32): per coordinate the ``keep`` consecutive
    sorted values closest to the median are averaged in ascending order (the window
    slides to where the values cluster; a tie keeps the lower value).  keep = K is
    ``trimmed_mean`` with trim 0, keep = 1 with an odd K the (finite, non-zero) median.  The client
    weights play no part.  U: fp32 [*, ld] rows with unit element stride; rows: int32
    [K], 1 <= K <= ROBUST_MAX_K; 1 <= keep <= K; P a multiple of 4, at most the row
    length."""
    fn = "mean_around_median"
    K, P, ldu = _rows_operands(fn, U, rows, P)
    keep = int(keep)
    if not 1 <= keep <= K:
        raise RuntimeError(f"{fn}: keep={keep} (1 <= keep <= K={K})")
    return _to_one_row(fn, U, ldu, rows, K, keep, P, out, stream)


def craft_rows(U, hrows, arows, a, b, P, base=None, stream=None):
    """Byzantine rows crafted in place from the honest rows of U (dls_craft_rows_f32):
    per coordinate out = base + a * (mu - base) + b * sigma, mu the ascending mean and
    sigma the population standard deviation of the Kh = hrows.numel() honest values
    (sigma only when b != 0; without ``base``, out = a * mu + b * sigma), written into
    each of the Ka = arows.numel() attacker rows.  Multiply, then add, every operation
    rounded once: the bits are those of the header's contract, the same for any order
    of ``hrows``.  hrows and arows: int32 [1..ROBUST_MAX_K] device tables that must not
    share a row (not checked here: the tables live on the device;
    ``ClientUpdateStore.craft`` checks its host lists); a, b finite; base: None or an
    fp32 vector of at least P elements; U, P as in pairwise_sqdist.  Returns U."""
    fn = "craft_rows"
    Kh, P, ldu = _rows_operands(fn, U, hrows, P)
    _rows_operands(fn, U, arows, P)
    a, b = float(a), float(b)
    if not (math.isfinite(a) and math.isfinite(b)):
        raise RuntimeError(f"{fn}: a={a} and b={b} must be finite")
    if base is not None:
        _f32_vector(fn, "base", base, P)
    _rows_placement(fn, U, ("base",), hrows=hrows, arows=arows, base=base)
    _ptr(U), _ptr(hrows), _ptr(arows), _ptr(base)  # no CPU path
    if P == 0:
        return U
    _check(lib().dls_craft_rows_f32(_ptr(U), ldu, _ptr(hrows), Kh, _ptr(arows), arows.numel(),
                                    a, b, _ptr(base), P, _stream(stream, U)),
           "dls_craft_rows_f32")
    return U


def rows_sqdist_to(U, rows, P, z, out=None, stream=None):
    """Squared Euclidean distances of the K = rows.numel() selected rows of U to the
    point z over their first P elements (dls_rows_sqdist_to_f32): an fp64 [K] device
    tensor, each entry within 2^-17 relative of the exact squared distance of the fp32
    operands; a row equal to z gives +0.0, rows of equal contents equal bits, a row
    that holds inf or NaN +inf or NaN (the other rows are unaffected).  U, rows, P as
    in pairwise_sqdist; z: fp32, at least P elements; out: a contiguous fp64 [K]
    tensor (default: a new one)."""
    fn = "rows_sqdist_to"
    K, P, ldu = _rows_operands(fn, U, rows, P)
    _f32_vector(fn, "z", z, P)
    _f64_out(fn, "out", out, (K,))
    _rows_placement(fn, U, ("z",), rows=rows, z=z, out=out)
    return _workspace_call("dls_rows_sqdist_to_f32", "dls_weiszfeld_workspace", K, P,
                           (U, ldu, rows, K, P, z), out, (K,), stream)


def _fused_step(fn, cname, U, rows, c, P, z, dist2, stream):
    """weiszfeld_step and centered_clip_step: dls_<fn>_f32 on the coefficients ``cname``."""
    K, P, ldu = _rows_operands(fn, U, rows, P)
    _k_tensor(fn, cname, c, torch.float32, (K,))
    _f32_vector(fn, "z", z, P)
    _f64_out(fn, "dist2", dist2, (K,))
    _rows_placement(fn, U, ("z",), rows=rows, **{cname: c}, z=z, dist2=dist2)
    return z, _workspace_call(f"dls_{fn}_f32", "dls_weiszfeld_workspace", K, P,
                              (U, ldu, rows, K, c, P, z), dist2, (K,), stream)


def weiszfeld_step(U, rows, w, P, z, dist2=None, stream=None):
    """One fused Weiszfeld step (dls_weiszfeld_step_f32): z[:P] = sum_k fl32(w[k] *
    U[rows[k]]) - multiply, then add in the order of ``rows``, every operation rounded
    once, so z is defined bit for bit by the bits of w - and the squared distances of
    the rows to that new z (as rows_sqdist_to) from the same read of the rows.  The
    old contents of z are never read.  w: a contiguous fp32 [K] tensor; the rest as in
    rows_sqdist_to.  Returns (z, dist2)."""
    return _fused_step("weiszfeld_step", "w", U, rows, w, P, z, dist2, stream)


def centered_clip_step(U, rows, c, P, z, dist2=None, stream=None):
    """One fused centered-clipping step (dls_centered_clip_step_f32), in place: z[:P] =
    fl32(z + sum_k fl32(c[k] * fl32(U[rows[k]] - z))) - subtract, multiply, add in the
    order of ``rows``, then add to z, every operation rounded once, so the new z is
    defined bit for bit by the bits of c and of the old z - and the squared distances
    of the rows to that new z (as rows_sqdist_to) from the same read of the rows.  c: a
    contiguous fp32 [K] tensor (the callers' min(1, tau / distance) / K); the rest as
    in rows_sqdist_to.  Returns (z, dist2)."""
    return _fused_step("centered_clip_step", "c", U, rows, c, P, z, dist2, stream)


# ------------------------------------------- the random stream and the DP-FedAvg step
NORMAL_MAX = math.sqrt(48.0 * math.log(2.0))  # |g| of the stream's normals never exceeds it


def _uint64(fn, name, v):
    """int(v); RuntimeError unless v is an integer in 0..2^64 - 1."""
    if isinstance(v, bool) or not isinstance(v, int) or not 0 <= v < 1 << 64:
        raise RuntimeError(f"{fn}: {name}={v!r} must be an integer in 0..2^64 - 1")
    return v


def _stream_range(fn, n, first):
    n, first = int(n), int(first)
    if n < 0 or first < 0 or first + n > (1 << 63) - 1:
        raise RuntimeError(f"{fn}: n={n} and first={first} must be non-negative, "
                           "first + n <= 2^63 - 1")
    return n, first


def _philox(fn, dtype, n, seed, stream_id, first, out, device, stream):
    n, first = _stream_range(fn, n, first)
    seed, stream_id = _uint64(fn, "seed", seed), _uint64(fn, "stream_id", stream_id)
    if out is None:
        if device is None:
            raise RuntimeError(f"{fn}: out or device is needed")
        out = torch.empty(n, dtype=dtype, device=device)
    _unit_vector(fn, "out", out, dtype, n, count=("n", n))
    _ptr(out)  # no CPU path
    if n != 0:
        _check(getattr(lib(), f"dls_{fn}")(_ptr(out), n, seed, stream_id, first,
                                           _stream(stream, out)), f"dls_{fn}")
    return out


def philox_u32(n, seed, stream_id, first=0, out=None, device=None, stream=None):
    """The words of the library's random stream (dls_philox_u32): out[i] is the Philox4x32-10
    word of coordinate first + i under (seed, stream_id), i < n; exact, a function of (seed,
    stream_id, coordinate) alone.  The bit pattern is held as int32 (torch has no arithmetic
    on uint32): view the numpy array as uint32.  seed, stream_id: integers in 0..2^64 - 1;
    out: an int32 vector of at least n elements (default: a new one on ``device``)."""
    return _philox("philox_u32", torch.int32, n, seed, stream_id, first, out, device, stream)


def philox_normal(n, seed, stream_id, first=0, out=None, device=None, stream=None):
    """The standard normals of the same coordinates (dls_philox_normal_f32): Box-Muller on
    the word pairs of a block, |g| <= NORMAL_MAX = sqrt(48 ln 2) ~ 5.768 (the tail is
    truncated there).  out: an fp32 vector of at least n elements (default: a new one on
    ``device``)."""
    return _philox("philox_normal_f32", torch.float32, n, seed, stream_id, first, out, device,
                   stream)


def normal_from_bits(bits, out=None, stream=None):
    """The Box-Muller transform alone (dls_normal_from_bits_f32) on caller-chosen words:
    (out[2j], out[2j+1]) from the word pair (bits[2j], bits[2j+1]).  bits: an int32 vector
    (the words' bit patterns) of an even number of elements; out: an fp32 vector of at least
    as many (default: a new one)."""
    fn = "normal_from_bits"
    _check_tensor(fn, "bits", bits, torch.int32, 0, "an int32 vector with unit stride",
                  exact=False, contiguous=False)
    n = bits.numel()
    if n % 2 != 0:
        raise RuntimeError(f"{fn}: bits holds n={n} words, not word pairs")
    if out is None:
        out = torch.empty(n, dtype=torch.float32, device=bits.device)
    _unit_vector(fn, "out", out, torch.float32, n, count=("n", n))
    _check_same_device(fn, bits, _anchor="bits", out=out)
    _ptr(bits), _ptr(out)  # no CPU path
    if n != 0:
        _check(lib().dls_normal_from_bits_f32(_ptr(bits), n, _ptr(out), _stream(stream, bits)),
               "dls_normal_from_bits_f32")
    return out


def dp_clip_noise_step(U, rows, c, P, z, sigma, seed, stream_id, stream=None):
    """One fused DP-FedAvg step (dls_dp_clip_noise_step_f32), in place: z[:P] = fl32(y +
    fl32(sigma * g)) with y the new z of ``centered_clip_step`` from the same operands, bit
    for bit, and g[p] the normal ``philox_normal`` gives coordinate p under (seed,
    stream_id); sigma == 0 draws nothing and stores y.  sigma: finite, >= 0 (used as its
    fp32 value); seed, stream_id: integers in 0..2^64 - 1; the rest as in
    centered_clip_step, without distances.  Returns z."""
    fn = "dp_clip_noise_step"
    K, P, ldu = _rows_operands(fn, U, rows, P)
    _k_tensor(fn, "c", c, torch.float32, (K,))
    _f32_vector(fn, "z", z, P)
    if isinstance(sigma, bool) or not isinstance(sigma, (int, float)) \
            or not math.isfinite(fl32(sigma)) or sigma < 0:
        raise RuntimeError(f"{fn}: sigma={sigma!r} must be finite in fp32 and >= 0")
    seed, stream_id = _uint64(fn, "seed", seed), _uint64(fn, "stream_id", stream_id)
    _rows_placement(fn, U, ("z",), rows=rows, c=c, z=z)
    _check_disjoint({"U": U, "z": z[:P]}, f"{fn}: {{a}} and {{b}} overlap")
    _ptr(U), _ptr(rows), _ptr(c), _ptr(z)  # no CPU path
    if P != 0:
        _check(lib().dls_dp_clip_noise_step_f32(_ptr(U), ldu, _ptr(rows), K, _ptr(c), P, _ptr(z),
                                                fl32(sigma), seed, stream_id, _stream(stream, U)),
               "dls_dp_clip_noise_step_f32")
    return z


# ------------------------------------------------------------------ secure aggregation
def _int_in(fn, name, v, lo, hi, hi_text=None):
    """int(v); RuntimeError unless v is an integer in lo..hi."""
    if isinstance(v, bool) or not isinstance(v, int) or not lo <= v <= hi:
        raise RuntimeError(f"{fn}: {name}={v!r} must be an integer in {lo}..{hi_text or hi}")
    return v


def _stream_table(fn, name, t):
    """A table of stream ids: an int64 vector with unit stride that holds the uint64 ids' bit
    patterns (torch has no arithmetic on uint64), or None for none: returns (t, count)."""
    if t is None:
        return None, 0
    _check_tensor(fn, name, t, torch.int64, 0, "an int64 vector with unit stride (the uint64 "
                  "stream ids' bit patterns), or None", exact=False, contiguous=False)
    return (t, t.numel()) if t.numel() else (None, 0)


def _secagg_streams(fn, add_streams, sub_streams):
    add, n_add = _stream_table(fn, "add_streams", add_streams)
    sub, n_sub = _stream_table(fn, "sub_streams", sub_streams)
    if n_add + n_sub > SECAGG_MAX_STREAMS:
        raise RuntimeError(f"{fn}: {n_add} + {n_sub} streams (at most SECAGG_MAX_STREAMS="
                           f"{SECAGG_MAX_STREAMS})")
    return add, n_add, sub, n_sub


def _secagg_extent(fn, P):
    P = int(P)
    if P < 0 or P % 4 != 0:
        raise RuntimeError(f"{fn}: P={P} must be a non-negative multiple of 4")
    return P


def secagg_mask(w, base, P, frac_bits, bits, weight, add_streams, sub_streams, seed, y, stats,
                stream=None):
    """The client's fused encode + mask (dls_secagg_mask_f32): y[:P] = q * weight + the mask
    words of ``add_streams`` - those of ``sub_streams``, mod 2^32, with q = clamp(rintf(fl32(
    fl32(w - base) * 2^frac_bits)), -L, L), L = 2^(bits-1) - 1, and q = 0 where w - base is
    not finite; stats[0] += the saturated coordinates, stats[1] += the non-finite ones
    (added to: zero it first).  w, base: fp32 vectors of at least P elements; y: an int32
    vector of at least P (the uint32 bit patterns, as in ``philox_u32``); stats: int32 [2];
    the stream tables: int64 vectors (uint64 bit patterns) or None.  Exact.  Returns y."""
    fn = "secagg_mask"
    P = _secagg_extent(fn, P)
    _f32_vector(fn, "w", w, P)
    _f32_vector(fn, "base", base, P)
    _unit_vector(fn, "y", y, torch.int32, P, count=("P", P))
    _unit_vector(fn, "stats", stats, torch.int32, 2, exact=True)
    frac_bits = _int_in(fn, "frac_bits", frac_bits, 0, 126)
    bits = _int_in(fn, "bits", bits, 2, 31)
    weight = _int_in(fn, "weight", weight, 1, (1 << 32) - 1, "2^32 - 1")
    add, n_add, sub, n_sub = _secagg_streams(fn, add_streams, sub_streams)
    seed = _uint64(fn, "seed", seed)
    _check_same_device(fn, w, _anchor="w", base=base, y=y, stats=stats, add_streams=add,
                       sub_streams=sub)
    _aligned16(fn, w=w, base=base, y=y)
    _check_disjoint({"y": y[:P], "w": w[:P], "base": base[:P]}, f"{fn}: {{a}} and {{b}} overlap",
                    allowed=lambda a, b: "y" not in (a, b))
    _ptr(w), _ptr(base), _ptr(y), _ptr(stats), _ptr(add), _ptr(sub)  # no CPU path
    if P != 0:
        _check(lib().dls_secagg_mask_f32(_ptr(w), _ptr(base), P, frac_bits, bits, weight,
                                         _ptr(add), n_add, _ptr(sub), n_sub, seed, _ptr(y),
                                         _ptr(stats), _stream(stream, w)), "dls_secagg_mask_f32")
    return y


def secagg_unmask(Y, rows, add_streams, sub_streams, seed, base, frac_bits, total, P, out,
                  sum_out=None, stream=None):
    """The server's fused sum + mask recovery + decode (dls_secagg_unmask_f32): S = the sum
    of the K = rows.numel() selected rows of Y + the mask words of ``add_streams`` - those of
    ``sub_streams``, mod 2^32; out[:P] = fl32(base + (float)((double)(int32)S * 2^-frac_bits
    / total)); sum_out[:P] = S if given.  Y: an int32 [rows, ld] matrix (uint32 bit
    patterns); total: finite, >= 1 (used as fp64); out may be base.  Exact.  Returns out."""
    fn = "secagg_unmask"
    K, P, ldy = _rows_operands(fn, Y, rows, P, names=("Y", "rows"), dtype=torch.int32)
    _f32_vector(fn, "base", base, P)
    _f32_vector(fn, "out", out, P)
    if sum_out is not None:
        _unit_vector(fn, "sum_out", sum_out, torch.int32, P, count=("P", P))
    frac_bits = _int_in(fn, "frac_bits", frac_bits, 0, 126)
    if isinstance(total, bool) or not isinstance(total, (int, float)) \
            or not math.isfinite(total) or total < 1:
        raise RuntimeError(f"{fn}: total={total!r} must be finite and >= 1")
    add, n_add, sub, n_sub = _secagg_streams(fn, add_streams, sub_streams)
    seed = _uint64(fn, "seed", seed)
    _rows_placement(fn, Y, ("base", "out", "sum_out"), rows=rows, base=base, out=out,
                    sum_out=sum_out, add_streams=add, sub_streams=sub)
    outs = {"out": out[:P]} if sum_out is None else {"out": out[:P], "sum_out": sum_out[:P]}
    _check_disjoint({"Y": Y, **outs}, f"{fn}: {{a}} and {{b}} overlap")
    _ptr(Y), _ptr(rows), _ptr(base), _ptr(out), _ptr(sum_out), _ptr(add), _ptr(sub)  # no CPU path
    if P != 0:
        _check(lib().dls_secagg_unmask_f32(_ptr(Y), ldy, _ptr(rows), K, _ptr(add), n_add,
                                           _ptr(sub), n_sub, seed, _ptr(base), frac_bits,
                                           float(total), P, _ptr(out), _ptr(sum_out),
                                           _stream(stream, Y)), "dls_secagg_unmask_f32")
    return out


# DLS_SERVER_OPT_* (include/dls_hip.h): the kinds, and the launch shape of the step
SERVER_OPT_SGD, SERVER_OPT_ADAGRAD, SERVER_OPT_ADAM, SERVER_OPT_YOGI = range(4)
SERVER_OPT_KINDS = {"sgd": SERVER_OPT_SGD, "adagrad": SERVER_OPT_ADAGRAD,
                    "adam": SERVER_OPT_ADAM, "yogi": SERVER_OPT_YOGI}
SERVER_OPT_BLOCK = 256  # threads per block
SERVER_OPT_MAX_BLOCKS = 2048  # the grid's cap: further vectors are grid-strided
SERVER_OPT_UNROLL = 2  # 16-byte vectors (of 4 elements) per thread and visit


def fl32(x):
    """The fp32 value nearest to x (ties to even), as a Python float."""
    return ctypes.c_float(float(x)).value


def server_opt_coeffs(lr, beta1, beta2, tau):
    """The coefficients dls_server_opt_step_f32 is handed, as Python floats that hold
    fp32 values: (lr, beta1, omb1, beta2, omb2, tau), each of lr, beta1, beta2, tau
    rounded to fp32 once and omb = fl32(1.0 - float64(fl32(beta))).  RuntimeError if one
    of them is not finite after the rounding."""
    lr, beta1, beta2, tau = fl32(lr), fl32(beta1), fl32(beta2), fl32(tau)
    coeffs = (lr, beta1, fl32(1.0 - beta1), beta2, fl32(1.0 - beta2), tau)
    if not all(math.isfinite(c) for c in coeffs):
        raise RuntimeError(f"server_opt_step: lr={lr}, beta1={beta1}, beta2={beta2} and tau={tau} "
                           "must be finite in fp32")
    return coeffs


def server_opt_step(kind, agg, x, m, v, out, P, lr, beta1, beta2, tau, stream=None):
    """One fused server-optimizer step (dls_server_opt_step_f32): with d = fl32(agg - x),
    SERVER_OPT_SGD: m' = fl32(fl32(beta1 * m) + d), out = fl32(x + fl32(lr * m'));
    the adaptive kinds: m' = fl32(fl32(beta1 * m) + fl32(omb1 * d)), v' from d2 = fl32(d *
    d) - ADAGRAD v + d2, ADAM fl32(beta2 * v) + fl32(omb2 * d2), YOGI v - fl32(omb2 *
    d2) * sign(v - d2) - and out = fl32(x + fl32(lr * m') / fl32(sqrt(v') + tau)), every
    operation rounded once, with the coefficients of ``server_opt_coeffs(lr, beta1,
    beta2, tau)``: numpy float32 reproduces out, m' and v' bit for bit.  agg, x, m, v,
    out: fp32 vectors of at least P elements with unit stride on one device; m and v
    are updated in place; v is None for SGD, m may be None for SGD with beta1 == 0;
    out may be x itself (the same first element) and nothing else may overlap.  Returns
    out."""
    fn = "server_opt_step"
    if isinstance(kind, bool) or not isinstance(kind, int) or not 0 <= kind <= SERVER_OPT_YOGI:
        raise RuntimeError(f"{fn}: kind={kind!r} must be one of {SERVER_OPT_KINDS}")
    P = int(P)
    if P < 0:
        raise RuntimeError(f"{fn}: P={P}")
    lr, beta1, omb1, beta2, omb2, tau = server_opt_coeffs(lr, beta1, beta2, tau)
    sgd = kind == SERVER_OPT_SGD
    if sgd and v is not None:
        raise RuntimeError(f"{fn}: v must be None for SERVER_OPT_SGD")
    if not sgd and v is None:
        raise RuntimeError(f"{fn}: kind={kind} needs v")
    if m is None and not (sgd and beta1 == 0.0):
        raise RuntimeError(f"{fn}: m may be None for SERVER_OPT_SGD with beta1 == 0 alone")
    ops = {"agg": agg, "x": x, "m": m, "v": v, "out": out}
    given = {name: t for name, t in ops.items() if not (t is None and name in ("m", "v"))}
    for name, t in given.items():
        _f32_vector(fn, name, t, P)
    _check_same_device(fn, agg, _anchor="agg", **given)
    _check_disjoint({name: t[:P] for name, t in given.items()},
                    f"{fn}: {{a}} and {{b}} overlap (out may be x itself, nothing else may overlap)",
                    allowed=lambda a, b: (a, b) == ("x", "out") and x.data_ptr() == out.data_ptr())
    for t in given.values():
        _ptr(t)  # no CPU path
    if P == 0:
        return out
    _check(lib().dls_server_opt_step_f32(kind, _ptr(agg), _ptr(x), _ptr(m), _ptr(v), _ptr(out), P,
                                         lr, beta1, omb1, beta2, omb2, tau, _stream(stream, agg)),
           "dls_server_opt_step_f32")
    return out


# ------------------------------------------------------- top-k sparsification
TOPK_MAX_P = (1 << 31) - 1  # idx is int32
# DLS_TOPK_* (include/dls_hip.h): the launch shape of dls_topk_compress_f32
TOPK_CHUNK = 4096  # coordinates per chunk (one block and trip)
TOPK_HIST_BLOCKS = 2048  # the histogram passes' grid cap: further chunks are grid-strided
TOPK_SCAN_BLOCK = 1024  # threads of the one scan block, ceil(chunks / it) chunks each


def _topk_extent(fn, P):
    P = int(P)
    if not 1 <= P <= TOPK_MAX_P or P % 4 != 0:
        raise RuntimeError(f"{fn}: P={P} must be a multiple of 4 in 4..2^31 - 4")
    return P


def topk_workspace(P, device):
    """The scratch buffer dls_topk_compress_f32 needs for rows of P elements (a uint8
    tensor on ``device``; its contents never matter between calls)."""
    P = _topk_extent("topk_workspace", P)
    nbytes = int(lib().dls_topk_workspace(P))
    if nbytes < 0:
        _check(nbytes, "dls_topk_workspace")
    return torch.empty(nbytes, dtype=torch.uint8, device=device)


def topk_compress(w, base, e, k, P, idx, val, stats, workspace, stream=None):
    """Top-k sparsification with error feedback (dls_topk_compress_f32): with u = fl32(
    fl32(w - base) + e), the k coordinates of the largest |u| (keys bits(u) & 0x7fffffff,
    ties to the lowest index) are written to idx[:k] (int32, strictly ascending) and
    val[:k] (u's bits); e becomes +0.0 there and u elsewhere; stats (int32 [2]) becomes
    (k, the number of non-finite u).  w, base, e: fp32 vectors of at least P elements
    with unit stride; idx / val: at least k elements; workspace: ``topk_workspace(P)``.
    1 <= k <= P, P a multiple of 4; e must not overlap w or base; w, base, e, idx, val
    and the workspace 16-byte aligned.  Nothing is synchronised: the outputs are ready in
    stream order.  Returns (idx, val)."""
    fn = "topk_compress"
    P = _topk_extent(fn, P)
    if isinstance(k, bool) or not isinstance(k, int) or not 1 <= k <= P:
        raise RuntimeError(f"{fn}: k={k!r} must be an integer in 1..P={P}")
    for name, t in (("w", w), ("base", base), ("e", e)):
        _f32_vector(fn, name, t, P)
    _unit_vector(fn, "idx", idx, torch.int32, k)
    _unit_vector(fn, "val", val, torch.float32, k)
    _unit_vector(fn, "stats", stats, torch.int32, 2)
    need = int(lib().dls_topk_workspace(P))
    _check_tensor(fn, "workspace", workspace, torch.uint8, need, lambda: "a uint8 vector of at "
                  f"least {need} bytes (topk_workspace(P))", exact=False, contiguous=False)
    _check_same_device(fn, w, _anchor="w", base=base, e=e, idx=idx, val=val, stats=stats,
                       workspace=workspace)
    for name, other in (("w", w), ("base", base)):
        if _overlaps(e[:P], other[:P]):
            raise RuntimeError(f"{fn}: e and {name} overlap (the residual is updated in place)")
    _check_disjoint({"e": e[:P], "idx": idx[:k], "val": val[:k], "stats": stats[:2],
                     "workspace": workspace}, f"{fn}: {{a}} and {{b}} overlap")
    for name, t in (("w", w), ("base", base), ("e", e), ("idx", idx), ("val", val),
                    ("workspace", workspace)):
        _aligned16(fn, **{name: t})
    for t in (w, base, e, idx, val, stats, workspace):
        _ptr(t)  # no CPU path
    _check(lib().dls_topk_compress_f32(_ptr(w), _ptr(base), _ptr(e), P, k, _ptr(idx), _ptr(val),
                                       _ptr(stats), _ptr(workspace), _stream(stream, w)),
           "dls_topk_compress_f32")
    return idx, val


def sparse_fedavg(base, idx, val, off, weight, total, P, out, stream=None):
    """FedAvg over sparse client updates, added to ``base`` (dls_sparse_fedavg_f32): client
    i of the K = weight.numel() clients, in the given order, holds the pairs idx / val[
    off[i]:off[i + 1]], its indices strictly ascending in 0..P-1.  A coordinate nobody
    sent keeps base's bits; elsewhere out = fl32(base + acc), acc the FedAvg chain
    fl32(fl32(v * n_i) / N) over its senders in client order (the first assigns, the
    rest add).  base, out: fp32 vectors of at least P elements with unit stride, 16-byte
    aligned, not overlapping; idx int32 / val fp32 of one length; off int64 [K + 1] with
    off[0] = 0 and off[K] = idx.numel() (the caller's word: it lives on the device);
    weight fp32 [K] = the n_i, total = their fp32 sum.  Returns out."""
    fn = "sparse_fedavg"
    P = _topk_extent(fn, P)
    _f32_vector(fn, "base", base, P)
    _f32_vector(fn, "out", out, P)
    # 1-D with unit stride and at least one element: contiguous [K], K >= 1
    _check_tensor(fn, "weight", weight, torch.float32, 1, "a contiguous fp32 [K] tensor, K >= 1",
                  exact=False, contiguous=False)
    K = weight.numel()
    _unit_vector(fn, "off", off, torch.int64, K + 1, exact=True)
    if not torch.is_tensor(idx) or not torch.is_tensor(val):
        raise RuntimeError(f"{fn}: idx and val must be tensors")
    _unit_vector(fn, "idx", idx, torch.int32, idx.numel() if idx.dim() == 1 else -1, exact=True)
    _unit_vector(fn, "val", val, torch.float32, idx.numel(), exact=True)
    total = fl32(total)
    if not math.isfinite(total) or total <= 0.0:
        raise RuntimeError(f"{fn}: total={total} must be a positive finite number")
    _check_same_device(fn, base, _anchor="base", idx=idx, val=val, off=off, weight=weight, out=out)
    if _overlaps(out[:P], base[:P]):
        raise RuntimeError(f"{fn}: out and base overlap (untouched coordinates are copied)")
    for name, t in (("idx", idx), ("val", val), ("off", off), ("weight", weight)):
        if t.numel() and _overlaps(out[:P], t):
            raise RuntimeError(f"{fn}: out and {name} overlap")
    _aligned16(fn, base=base, out=out)
    for t in (base, idx, val, off, weight, out):
        _ptr(t)  # no CPU path
    has = idx.numel() > 0  # an empty tensor's pointer means nothing: hand the library null
    _check(lib().dls_sparse_fedavg_f32(_ptr(base), _ptr(idx) if has else None,
                                       _ptr(val) if has else None, _ptr(off), _ptr(weight), K,
                                       total, P, _ptr(out), _stream(stream, base)),
           "dls_sparse_fedavg_f32")
    return out


def subset_fedavg(U, sub_off, sub_rows, sub_weight, sub_total, P, out, stream=None):
    S = sub_off.numel() - 1
    _check(lib().dls_subset_fedavg_f32(_ptr(U), U.stride(0), _ptr(sub_off), _ptr(sub_rows),
                                       _ptr(sub_weight), _ptr(sub_total), S, P, _ptr(out),
                                       out.stride(0), _stream(stream, U)), "dls_subset_fedavg_f32")
    return out


def subset_fedavg_union(U, urows, uweight, member, sub_total, P, out, stream=None):
    """S <= SUBSET_UNION_MAX coalitions over one client union, each client row read
    once (dls_subset_fedavg_union_f32); member: int64 [Ku] bit masks (device);
    sub_total: the S divisors fl32(N_s) (host: a sequence of numbers)."""
    assert urows.dtype == torch.int32 and uweight.dtype == torch.float32
    assert member.dtype == torch.int64
    tot = [float(x) for x in sub_total]
    S = len(tot)
    _check(lib().dls_subset_fedavg_union_f32(_ptr(U), U.stride(0), _ptr(urows), _ptr(uweight),
                                             _ptr(member), urows.numel(), (ctypes.c_float * S)(*tot),
                                             S, P, _ptr(out), out.stride(0), _stream(stream, U)),
           "dls_subset_fedavg_union_f32")
    return out


def subset_gemm(C, U, rows, P, out, stream=None):
    S, K = C.shape
    assert C.is_contiguous() and C.dtype == torch.float32
    _check(lib().dls_subset_gemm_f32(_ptr(C), S, K, _ptr(U), U.stride(0), _ptr(rows), P, _ptr(out),
                                     out.stride(0), _stream(stream, U)), "dls_subset_gemm_f32")
    return out


# ------------------------------------------------------------------------ sign
def sign_pack(X, P, planes, nonternary=None, stream=None):
    K = X.shape[0]
    _check(lib().dls_sign_pack_f32(_ptr(X), X.stride(0), K, P, _ptr(planes), planes.stride(0),
                                   _ptr(nonternary), _stream(stream, X)), "dls_sign_pack_f32")
    return planes


def sign_vote_count(planes, rows, K, P, counts, stream=None):
    _check(lib().dls_sign_vote_count(_ptr(planes), planes.stride(0), _ptr(rows), K, P,
                                     _ptr(counts), _stream(stream, planes)), "dls_sign_vote_count")
    return counts


def sign_from_counts(counts, P, sign_out=None, vote_planes=None, stream=None):
    _check(lib().dls_sign_from_counts(_ptr(counts), P, _ptr(sign_out), _ptr(vote_planes),
                                      _stream(stream, counts)), "dls_sign_from_counts")


def sign_vote(planes, rows, K, P, sign_out, counts=None, vote_planes=None, stream=None):
    """Fused vote (dls_sign_vote): any of fp32 signs, int32 counts, packed vote."""
    _check(lib().dls_sign_vote(_ptr(planes), planes.stride(0), _ptr(rows), K, P, _ptr(counts),
                               _ptr(sign_out), _ptr(vote_planes), _stream(stream, planes)),
           "dls_sign_vote")
    return sign_out


def _require_logical_f32(fn, **tensors):
    """The worker kernels walk memory from data_ptr() for numel() elements: every
    tensor must be fp32 with its memory in logical (row-major) order."""
    for name, t in tensors.items():
        if t is None:
            continue
        if t.dtype != torch.float32 or not t.is_contiguous():
            raise RuntimeError(f"{fn}: {name} must be a contiguous fp32 tensor (memory in logical "
                               f"order), not {t.dtype} with shape {tuple(t.shape)} and strides "
                               f"{tuple(t.stride())}")


def _require_plane_words(fn, planes, P):
    """planes: int64 words with unit stride, at least the 2 * ceil(P / 64) the kernel touches."""
    need = 2 * ((P + 63) // 64)
    if planes.dtype != torch.int64 or planes.dim() != 1 or not planes.is_contiguous() \
            or planes.numel() < need:
        raise RuntimeError(f"{fn}: planes must be a contiguous int64 vector of at least {need} "
                           f"words for {P} parameters, not {planes.dtype} "
                           f"{tuple(planes.shape)}")


def sign_sgd_direction(grad, buf, momentum, one_minus_dampening, nesterov, first, planes,
                       sign_out=None, stream=None):
    """workers/sign_sgd_worker.py:32-44 on one tensor (dls_sign_sgd_direction): updates
    ``buf`` in place and writes the 2 * ceil(P / 64) plane words of the signs to
    ``planes``.  grad, buf and sign_out hold P elements each in logical order."""
    fn = "sign_sgd_direction"
    P = grad.numel()
    _require_logical_f32(fn, grad=grad, buf=buf, sign_out=sign_out)
    for name, t in (("buf", buf), ("sign_out", sign_out)):
        if t is not None and t.numel() != P:
            raise RuntimeError(f"{fn}: {name} holds {t.numel()} elements, grad {P}")
    _require_plane_words(fn, planes, P)
    _check(lib().dls_sign_sgd_direction(_ptr(grad), _ptr(buf), P, float(momentum),
                                        float(one_minus_dampening), int(bool(nesterov)),
                                        int(bool(first)), _ptr(planes), _ptr(sign_out),
                                        _stream(stream, grad)), "dls_sign_sgd_direction")


def sign_sgd_apply(param, vote_planes, neg_lr, weight_decay, stream=None):
    """workers/sign_sgd_worker.py:48-57 on one tensor, in place (dls_sign_sgd_apply).
    Bit j of the vote's group g is the parameter's element 64 g + j in memory, so
    ``param`` must have its memory in logical order: a tensor that has not (a
    channels_last weight) is rejected, not stepped with a permuted vote."""
    fn = "sign_sgd_apply"
    _require_logical_f32(fn, param=param)
    _require_plane_words(fn, vote_planes, param.numel())
    _check(lib().dls_sign_sgd_apply(_ptr(param), _ptr(vote_planes), param.numel(), float(neg_lr),
                                    float(weight_decay), _stream(stream, param)), "dls_sign_sgd_apply")


# ----------------------------------------------------------------------- quant
def dequant_fedavg(tiles, ntiles, nfast, Q, F, sz, rows, weight, total, out, sz_strides=None,
                   mode=FEDAVG_EXACT, stream=None):
    """nfast: the QTILE_GROUPS counts of grouped tiles at the head of the table
    (quant_store.QuantLayout.tiles()); sz: (scale, zero point) pairs;
    sz_strides = (row, channel) strides in pairs (default: a channel-major
    [C+1, capacity, 2] tensor)."""
    assert len(nfast) == QTILE_GROUPS
    nf = (ctypes.c_int32 * QTILE_GROUPS)(*[int(x) for x in nfast])
    if sz_strides is None:
        sz_strides = (sz.stride(1) // 2, sz.stride(0) // 2)
    _check(lib().dls_dequant_fedavg_mode(_ptr(tiles), ntiles, nf, _ptr(Q),
                                         Q.stride(0) if Q is not None else 0,
                                         _ptr(F), F.stride(0) if F is not None else 0, _ptr(sz),
                                         int(sz_strides[0]), int(sz_strides[1]), _ptr(rows),
                                         _ptr(weight), rows.numel(), float(total), int(mode),
                                         _ptr(out), _stream(stream, out)), "dls_dequant_fedavg")
    return out


def segment_minmax(x, seg_off, total, mins, maxs, stream=None):
    _check(lib().dls_segment_minmax_f32(_ptr(x), _ptr(seg_off), seg_off.numel() - 1, _ptr(mins),
                                        _ptr(maxs), total, _stream(stream, x)),
           "dls_segment_minmax_f32")


def qparams_minmax(mins, maxs, scale, zp, qmin=0, qmax=255, symmetric=False, stream=None):
    _check(lib().dls_qparams_minmax(_ptr(mins), _ptr(maxs), mins.numel(), qmin, qmax,
                                    int(bool(symmetric)), _ptr(scale), _ptr(zp),
                                    _stream(stream, mins)), "dls_qparams_minmax")


def quantize(x, seg_off, total, scale, zp, q, deq=None, qmin=0, qmax=255, stochastic=False,
             seed=0, stream=None):
    _check(lib().dls_quantize_affine(_ptr(x), _ptr(seg_off), seg_off.numel() - 1, _ptr(scale),
                                     _ptr(zp), qmin, qmax, _ptr(q), _ptr(deq),
                                     int(bool(stochastic)),
                                     ctypes.c_uint64(seed & 0xFFFFFFFFFFFFFFFF), total,
                                     _stream(stream, x)), "dls_quantize_affine")


def quantize_u8(x, seg_off, total, scale, zp, q, deq=None, stochastic=False, seed=0,
                stream=None, qmax=255):
    """Unsigned bytes in [0, qmax] (qmax = levels - 1 of the qparams)."""
    quantize(x, seg_off, total, scale, zp, q, deq, 0, qmax, stochastic, seed, stream)


# ----------------------------------------------------------- utility evaluation
# The kernels index their operands from the shapes alone, so the wrappers refuse
# whatever would send them out of bounds before any pointer reaches the library.

def _check_f32_vector(fn, name, t, n, device):
    _check_tensor(fn, name, t, torch.float32, n,
                  lambda: f"a contiguous fp32 tensor of {n} elements on {device}", device=device)


def _check_bn_module(fn, bn, device):
    """The module's tensors: fp32 [C], contiguous, on the outputs' device (weight and
    bias may be None: affine=False)."""
    C = int(bn.num_features)
    if C <= 0:
        raise RuntimeError(f"{fn}: num_features = {C}")
    for name in ("running_mean", "running_var", "weight", "bias"):
        t = getattr(bn, name)
        if t is None and name in ("weight", "bias"):
            continue
        _check_f32_vector(fn, f"bn.{name}", t, C, device)
    return C


def _check_bn_activations(fn, x, residual, out, memory_format, layout):
    """x: fp32 [N, C, H, W] in the given layout; residual and out: x's shape, dtype,
    layout and device."""
    if x.dim() != 4 or x.dtype != torch.float32:
        raise RuntimeError(f"{fn}: x must be an fp32 [N, C, H, W] tensor, got {x.dtype} "
                           f"{tuple(x.shape)}")
    for name, t in (("x", x), ("residual", residual), ("out", out)):
        if t is None:
            continue
        if t.shape != x.shape or t.dtype != x.dtype or t.device != x.device:
            raise RuntimeError(f"{fn}: {name} must have x's shape, dtype and device "
                               f"({tuple(x.shape)}, {x.dtype}, {x.device}), got {tuple(t.shape)}, "
                               f"{t.dtype}, {t.device}")
        if not t.is_contiguous(memory_format=memory_format):
            raise RuntimeError(f"{fn}: activations must be {layout} contiguous ({name} is not)")


def bn_fold(bn, alpha, beta, stream=None):
    """Eval-mode constants of a BatchNorm module (dls_bn_fold_f32) into alpha, beta [C]."""
    C = _check_bn_module("bn_fold", bn, alpha.device)
    _check_f32_vector("bn_fold", "alpha", alpha, C, alpha.device)
    _check_f32_vector("bn_fold", "beta", beta, C, alpha.device)
    _check(lib().dls_bn_fold_f32(_ptr(bn.weight), _ptr(bn.bias), _ptr(bn.running_mean),
                                 _ptr(bn.running_var), float(bn.eps), C,
                                 _ptr(alpha), _ptr(beta), _stream(stream, alpha)),
           "dls_bn_fold_f32")


def bn_act_nhwc(x, alpha, beta, residual=None, relu=True, out=None, inplace=False, stream=None):
    """y = act(x * alpha + beta [+ residual]) over a channels_last [N, C, H, W] fp32
    activation in one pass (dls_bn_act_nhwc_f32); returns y (channels_last;
    x itself when inplace).  out may be x or residual."""
    cl = torch.channels_last
    _check_bn_activations("bn_act_nhwc", x, residual, out, cl, "channels_last")
    N, C, H, W = x.shape
    _check_f32_vector("bn_act_nhwc", "alpha", alpha, C, x.device)
    _check_f32_vector("bn_act_nhwc", "beta", beta, C, x.device)
    if out is None:
        out = x if inplace else torch.empty_like(x, memory_format=cl)
    _check(lib().dls_bn_act_nhwc_f32(_ptr(x), N * H * W, C, _ptr(alpha), _ptr(beta),
                                     _ptr(residual), int(bool(relu)), _ptr(out),
                                     _stream(stream, x)), "dls_bn_act_nhwc_f32")
    return out


def bn_fold_exact(bn, consts, stream=None):
    """The GPU library's eval batch-norm constants of a BatchNorm module into
    consts [4*C] = [mean | iv | w | b] (dls_bn_fold_exact_f32)."""
    C = _check_bn_module("bn_fold_exact", bn, consts.device)
    _check_f32_vector("bn_fold_exact", "consts", consts, 4 * C, consts.device)
    _check(lib().dls_bn_fold_exact_f32(_ptr(bn.weight), _ptr(bn.bias), _ptr(bn.running_mean),
                                       _ptr(bn.running_var), float(bn.eps), C,
                                       _ptr(consts), _stream(stream, consts)),
           "dls_bn_fold_exact_f32")


def bn_act_exact_nhwc(x, consts, residual=None, relu=True, out=None, inplace=False, stream=None):
    """y = act(fma(w, (x - mean) * iv, b) [+ residual]) over a channels_last
    [N, C, H, W] fp32 activation in one pass (dls_bn_act_exact_nhwc_f32)."""
    cl = torch.channels_last
    _check_bn_activations("bn_act_exact_nhwc", x, residual, out, cl, "channels_last")
    N, C, H, W = x.shape
    _check_f32_vector("bn_act_exact_nhwc", "consts", consts, 4 * C, x.device)
    if out is None:
        out = x if inplace else torch.empty_like(x, memory_format=cl)
    _check(lib().dls_bn_act_exact_nhwc_f32(_ptr(x), N * H * W, C, _ptr(consts), _ptr(residual),
                                           int(bool(relu)), _ptr(out),
                                           _stream(stream, x)), "dls_bn_act_exact_nhwc_f32")
    return out


def bn_act_exact_nchw(x, consts, residual=None, relu=True, out=None, inplace=False, stream=None):
    """bn_act_exact_nhwc over an NCHW-contiguous [N, C, H, W] fp32 activation
    (dls_bn_act_exact_nchw_f32: float4 planes when H*W is a multiple of 4 and every
    activation pointer is 16-byte aligned, one element per lane otherwise)."""
    _check_bn_activations("bn_act_exact_nchw", x, residual, out, torch.contiguous_format, "NCHW")
    N, C, H, W = x.shape
    _check_f32_vector("bn_act_exact_nchw", "consts", consts, 4 * C, x.device)
    if out is None:
        out = x if inplace else torch.empty_like(x, memory_format=torch.contiguous_format)
    _check(lib().dls_bn_act_exact_nchw_f32(_ptr(x), N, C, H * W, _ptr(consts), _ptr(residual),
                                           int(bool(relu)), _ptr(out),
                                           _stream(stream, x)), "dls_bn_act_exact_nchw_f32")
    return out


def bn_act_exact(x, consts, residual=None, relu=True, out=None, inplace=False, stream=None):
    """The exact eval batch-norm pass in the activation's own layout: channels_last
    (NHWC) or contiguous (NCHW)."""
    if x.is_contiguous(memory_format=torch.channels_last) and not x.is_contiguous():
        return bn_act_exact_nhwc(x, consts, residual, relu, out, inplace, stream)
    return bn_act_exact_nchw(x, consts, residual, relu, out, inplace, stream)


# ------------------------------------------------ deterministic convolutions
# "split" tensors (csrc/conv.hip): an fp32 value as a bf16 pair (hi, lo), stored
# as int16 — activations [B, H, W, 2C] (per pixel C hi then C lo), weights
# [Cout, 2K] (K hi then K lo, k = (ky*KW + kx)*Cp + ci).

def _check_consts(fn, consts, cout, device):
    """Eval batch-norm constants [mean | iv | w | b] x Cout: the kernels read them as
    16-byte vectors at consts + t * Cout + co."""
    if consts is None:
        return
    if (consts.dtype != torch.float32 or consts.numel() != 4 * cout or not consts.is_contiguous()
            or consts.device != device):
        raise RuntimeError(f"{fn}: consts must be a contiguous fp32 tensor of 4 * Cout = {4 * cout} "
                           f"elements on {device}")


def _check_nchw(fn, x, what="x must be a contiguous NCHW fp32 tensor"):
    if x.dtype != torch.float32 or x.dim() != 4 or not x.is_contiguous():
        raise RuntimeError(f"{fn}: {what}")
    return x.shape


_WEIGHTS_4D = "w must be a contiguous fp32 [Cout, Cin, KH, KW]"


def _conv_out_hw(H, W, ksize, stride, pad):
    return (H + 2 * pad - ksize[0]) // stride + 1, (W + 2 * pad - ksize[1]) // stride + 1


def split_channels(c):
    """The padded channel count of a split tensor: a multiple of 32."""
    return (int(c) + 31) // 32 * 32


# DLS_CONV_KERNEL_* / DLS_STEM_KERNEL_* (include/dls_hip.h): id -> kernel instantiation
CONV_KERNELS = {
    0: "none", 1: "generic<1,4>", 2: "generic<2,2>", 3: "pipe<1,4,10,1,2>", 4: "pipe<1,4,12,1,2>",
    5: "pipe<2,2,5,1,2>", 6: "pipe<2,4,5>", 7: "pipe<2,4,6>", 8: "halo<2,2,9,false>",
    9: "halo<2,2,9,true>", 10: "halo<1,4,11,false>", 11: "halo<1,4,11,true>", 12: "phase<2,4,5>",
}
STEM_KERNELS = {0: "none", 1: "window", 2: "3x3", 3: "generic"}


def conv_kernel_choice(B, H, W, C, Cout, ksize, stride, pad):
    """The kernel id (CONV_KERNELS) conv_bn_act launches for a shape, or the negative
    status it would fail with (dls_conv_kernel_choice: host only, needs no GPU)."""
    kh, kw = ksize
    return int(lib().dls_conv_kernel_choice(B, H, W, C, Cout, kh, kw, stride, pad))


def conv_stem_kernel_choice(B, C, H, W, Cout, ksize, stride, pad):
    """The kernel id (STEM_KERNELS) conv_stem_bn_act launches for a shape, or the
    negative status it would fail with (dls_conv_stem_kernel_choice: host only)."""
    kh, kw = ksize
    return int(lib().dls_conv_stem_kernel_choice(B, C, H, W, Cout, kh, kw, stride, pad))


def sign_vote_geometry(P, K, cus=0):
    """(nwaves, G, waves per block) of the sign_vote / sign_vote_count launch for P
    parameters and K client rows on a part with ``cus`` compute units (0: the current
    device; an explicit count needs no GPU): nwaves waves each own a contiguous
    range of at most 64 G vote groups of 64 parameters (dls_sign_vote_geometry,
    host only; the launch runs the same function)."""
    nwaves, G, wpb = ctypes.c_int64(), ctypes.c_int32(), ctypes.c_int32()
    _check(lib().dls_sign_vote_geometry(int(P), int(K), int(cus), ctypes.byref(nwaves),
                                        ctypes.byref(G), ctypes.byref(wpb)),
           "dls_sign_vote_geometry")
    return nwaves.value, G.value, wpb.value


def sign_vote_wave_ranges(P, K, cus=0, first_wave=0, count=None):
    """The vote-group ranges [wlo, whi) of ``count`` waves from ``first_wave`` (default:
    all of them) as two int64 numpy arrays, from the range function k_sign_vote itself
    calls (dls_sign_vote_wave_ranges, host only)."""
    import numpy as np
    if count is None:
        count = sign_vote_geometry(P, K, cus)[0] - first_wave
    wlo, whi = np.empty(count, np.int64), np.empty(count, np.int64)
    _check(lib().dls_sign_vote_wave_ranges(int(P), int(K), int(cus), int(first_wave), int(count),
                                           wlo.ctypes.data, whi.ctypes.data),
           "dls_sign_vote_wave_ranges")
    return wlo, whi


def conv_pack_input(x, stream=None):
    """NCHW fp32 [B, C, H, W] -> split NHWC [B, H, W, 2 Cp] (zeros beyond C)."""
    B, C, H, W = _check_nchw("conv_pack_input", x)
    cp = split_channels(C)
    out = torch.empty((B, H, W, 2 * cp), dtype=torch.int16, device=x.device)
    _check(lib().dls_conv_pack_input_f32(_ptr(x), B, C, H, W, cp, _ptr(out), _stream(stream, x)),
           "dls_conv_pack_input_f32")
    return out


def conv_pack_weights(w, stream=None):
    """fp32 [Cout, Cin, KH, KW] -> split weights [Cout, 2K] with K = KH*KW*Cp."""
    w = w.detach()
    co, ci, kh, kw = _check_nchw("conv_pack_weights", w, _WEIGHTS_4D)
    cp = split_channels(ci)
    out = torch.empty((co, 2 * kh * kw * cp), dtype=torch.int16, device=w.device)
    _check(lib().dls_conv_pack_weights_f32(_ptr(w), co, ci, kh, kw, cp, _ptr(out),
                                           _stream(stream, w)), "dls_conv_pack_weights_f32")
    return out


def conv_pack_im2col(x, ksize, stride, pad, stream=None):
    """NCHW fp32 [B, C, H, W] -> the split NHWC im2col [B, Ho, Wo, 2 Kp] of a
    (KH, KW) convolution, Kp = KH*KW*C rounded up to 32: the operand of a 1x1
    conv_bn_act with conv_pack_weights_im2col weights (few-channel first layers)."""
    B, C, H, W = _check_nchw("conv_pack_im2col", x)
    kh, kw = ksize
    kp = split_channels(kh * kw * C)
    ho, wo = _conv_out_hw(H, W, ksize, stride, pad)
    out = torch.empty((B, ho, wo, 2 * kp), dtype=torch.int16, device=x.device)
    _check(lib().dls_conv_pack_im2col_f32(_ptr(x), B, C, H, W, kh, kw, stride, pad, kp, _ptr(out),
                                          _stream(stream, x)), "dls_conv_pack_im2col_f32")
    return out


def conv_pack_weights_im2col(w, stream=None):
    """fp32 [Cout, Cin, KH, KW] -> split weights [Cout, 2 Kp] in conv_pack_im2col's k order."""
    w = w.detach()
    co, ci, kh, kw = _check_nchw("conv_pack_weights_im2col", w, _WEIGHTS_4D)
    kp = split_channels(kh * kw * ci)
    out = torch.empty((co, 2 * kp), dtype=torch.int16, device=w.device)
    _check(lib().dls_conv_pack_weights_im2col_f32(_ptr(w), co, ci, kh, kw, kp, _ptr(out),
                                                  _stream(stream, w)), "dls_conv_pack_weights_im2col_f32")
    return out


def conv_bn_act(x, w, ksize, stride, pad, consts=None, residual=None, relu=True, out=None,
                stream=None):
    """y = act(bn(conv(x)) [+ residual]) over split NHWC activations
    (dls_conv_bn_act_split); w from conv_pack_weights, ksize = (KH, KW)."""
    B, H, W, c2 = x.shape
    kh, kw = ksize
    cout = w.shape[0]
    ho, wo = _conv_out_hw(H, W, ksize, stride, pad)
    if x.dtype != torch.int16 or w.dtype != torch.int16 or not (x.is_contiguous() and w.is_contiguous()):
        raise RuntimeError("conv_bn_act: split int16 contiguous operands expected")
    if w.shape[1] != kh * kw * c2:
        raise RuntimeError(f"conv_bn_act: weights {tuple(w.shape)} do not match input channels {c2 // 2}")
    _check_same_device("conv_bn_act", x, w=w)
    _check_consts("conv_bn_act", consts, cout, x.device)
    oshape = (B, ho, wo, 2 * cout)
    if residual is not None:
        if (tuple(residual.shape) != oshape or residual.dtype != torch.int16
                or not residual.is_contiguous()):
            raise RuntimeError("conv_bn_act: residual must be a contiguous split NHWC int16 tensor "
                               "of the output's shape")
        _check_same_device("conv_bn_act", x, residual=residual)
    if out is None:
        out = torch.empty(oshape, dtype=torch.int16, device=x.device)
    else:
        if tuple(out.shape) != oshape or out.dtype != torch.int16 or not out.is_contiguous():
            raise RuntimeError(f"conv_bn_act: out must be a contiguous int16 tensor of shape {oshape}")
        _check_same_device("conv_bn_act", x, out=out)
        for name, t in (("x", x), ("residual", residual)):
            if t is not None and _overlaps(out, t):
                raise RuntimeError(f"conv_bn_act: out must not alias {name}")
    _check(lib().dls_conv_bn_act_split(_ptr(x), B, H, W, c2 // 2, _ptr(w), cout, kh, kw, stride,
                                       pad, _ptr(consts), _ptr(residual), int(bool(relu)),
                                       _ptr(out), _stream(stream, x)), "dls_conv_bn_act_split")
    return out


def conv_stem_bn_act(x, w, ksize, stride, pad, consts=None, relu=True, stream=None):
    """A few-channel first layer straight from the NCHW fp32 batch x (the im2col
    fused; KH*KW*C <= 32): y = act(bn(conv(x))) split NHWC
    (dls_conv_stem_bn_act_f32); w from conv_pack_weights_im2col."""
    B, C, H, W = _check_nchw("conv_stem_bn_act", x)
    kh, kw = ksize
    cout = w.shape[0]
    if w.dtype != torch.int16 or w.shape[1] != 2 * 32 or not w.is_contiguous():
        raise RuntimeError("conv_stem_bn_act: w must be conv_pack_weights_im2col output with Kp = 32")
    _check_same_device("conv_stem_bn_act", x, w=w)
    _check_consts("conv_stem_bn_act", consts, cout, x.device)
    ho, wo = _conv_out_hw(H, W, ksize, stride, pad)
    out = torch.empty((B, ho, wo, 2 * cout), dtype=torch.int16, device=x.device)
    _check(lib().dls_conv_stem_bn_act_f32(_ptr(x), B, C, H, W, _ptr(w), cout, kh, kw, stride, pad,
                                          _ptr(consts), int(bool(relu)), _ptr(out),
                                          _stream(stream, x)), "dls_conv_stem_bn_act_f32")
    return out


def pool_linear(x, weight, bias=None, stream=None):
    """Global average pool + linear layer over a split NHWC activation -> fp32
    logits [B, O] (dls_pool_linear_split)."""
    B, H, W, c2 = x.shape
    if x.dtype != torch.int16 or not x.is_contiguous():
        raise RuntimeError("pool_linear: x must be a contiguous split NHWC int16 tensor")
    if (weight.dim() != 2 or weight.shape[1] != c2 // 2 or weight.dtype != torch.float32
            or not weight.is_contiguous()):
        raise RuntimeError("pool_linear: weight must be a contiguous [O, C] fp32 tensor")
    O = weight.shape[0]
    if bias is not None and (tuple(bias.shape) != (O,) or bias.dtype != torch.float32
                             or not bias.is_contiguous()):
        raise RuntimeError("pool_linear: bias must be a contiguous [O] fp32 tensor")
    _check_same_device("pool_linear", x, weight=weight, bias=bias)
    out = torch.empty((B, O), dtype=torch.float32, device=x.device)
    _check(lib().dls_pool_linear_split(_ptr(x), B, H * W, c2 // 2, _ptr(weight.detach()),
                                       _ptr(None if bias is None else bias.detach()), O, _ptr(out),
                                       _stream(stream, x)), "dls_pool_linear_split")
    return out


# ------------------------------------------------- batched LeNet-5 evaluation
LENET5_MAX_OUT = 32  # fc3 outputs dls_lenet5_eval_f32 takes
LENET5_NAMES = ("conv1.weight", "conv1.bias", "conv2.weight", "conv2.bias", "fc1.weight",
                "fc1.bias", "fc2.weight", "fc2.bias", "fc3.weight", "fc3.bias")


def lenet5_shapes(num_out):
    """The ten parameter shapes of a LeNet-5 with num_out outputs, in LENET5_NAMES order."""
    return ((6, 1, 5, 5), (6,), (16, 6, 5, 5), (16,), (120, 400), (120,), (84, 120), (84,),
            (num_out, 84), (num_out,))


def _check_labels(fn, labels, B):
    if labels.dtype != torch.int64 or tuple(labels.shape) != (B,) or not labels.is_contiguous():
        raise RuntimeError(f"{fn}: labels must be a contiguous int64 [B] tensor")


def _loss_rows(fn, loss, S, B):
    """The row pitch of a per-image loss output: fp32 [S, B] with unit element
    stride, rows at any pitch >= B (a column window of a wider [S, n] buffer)."""
    if (loss.dtype != torch.float32 or tuple(loss.shape) != (S, B)
            or (B > 1 and loss.stride(1) != 1) or (S > 1 and loss.stride(0) < B)):
        raise RuntimeError(f"{fn}: loss must be fp32 [S, B] with unit element stride and a row "
                           "pitch of at least B")
    return _row_pitch(loss)


def softmax_ce(logits, labels, loss=None, stream=None):
    """Per-image cross-entropy of fp32 logits [S, B, O] (or [B, O]) against int64
    labels [B] (dls_softmax_ce_f32): fp32 [S, B], written into ``loss`` when given
    (see _loss_rows).  Any O >= 1; a label outside [0, O) gives NaN."""
    fn = "softmax_ce"
    if logits.dim() == 2:
        logits = logits.unsqueeze(0)
    if logits.dtype != torch.float32 or logits.dim() != 3 or not logits.is_contiguous():
        raise RuntimeError(f"{fn}: logits must be a contiguous fp32 [S, B, O] tensor")
    S, B, O = logits.shape
    _check_labels(fn, labels, B)
    if loss is None:
        loss = torch.empty((S, B), dtype=torch.float32, device=logits.device)
    _check_same_device(fn, logits, labels=labels, loss=loss)
    ldn = _loss_rows(fn, loss, S, B)
    _check(lib().dls_softmax_ce_f32(_ptr(logits), S, B, O, _ptr(labels), _ptr(loss), ldn,
                                    _stream(stream, logits)), "dls_softmax_ce_f32")
    return loss


def sum_rows_f64(v, out=None, stream=None):
    """out[s] = the fp64 sum of row s of the fp32 matrix v [S, n] (unit element
    stride, any row pitch >= n), in an order fixed by n alone (dls_sum_rows_f64).
    Returns fp64 [S]."""
    fn = "sum_rows_f64"
    if (v.dtype != torch.float32 or v.dim() != 2 or v.shape[0] < 1
            or (v.shape[1] > 1 and v.stride(1) != 1)
            or (v.shape[0] > 1 and v.stride(0) < v.shape[1])):
        raise RuntimeError(f"{fn}: v must be fp32 [S >= 1, n] with unit element stride")
    S, n = v.shape
    if out is None:
        out = torch.empty((S,), dtype=torch.float64, device=v.device)
    elif out.dtype != torch.float64 or tuple(out.shape) != (S,) or not out.is_contiguous():
        raise RuntimeError(f"{fn}: out must be a contiguous fp64 [S] tensor")
    _check_same_device(fn, v, out=out)
    ldn = _row_pitch(v)
    # an empty tensor may have no storage: nothing of v is read when n == 0, so any
    # valid device address serves
    vp = _ptr(v) if n > 0 or v.data_ptr() else _ptr(out)
    _check(lib().dls_sum_rows_f64(vp, ldn, S, n, _ptr(out), _stream(stream, v)),
           "dls_sum_rows_f64")
    return out


def lenet5_eval(models, offsets, x, labels=None, logits=None, correct=None, stream=None,
                num_out=None, loss=None):
    """S LeNet-5 models x B images in one launch (dls_lenet5_eval_f32).

    models: fp32 [S, ld] (or one row [ld]), a LeNet-5 per row in the flat layout;
    offsets: the ten element offsets of LENET5_NAMES within a row
    (ParameterLayout.offsets); x: fp32 [B, 1, 32, 32] contiguous; labels: int64
    [B] (needed for correct and loss).  Outputs, at least one: logits fp32 [S, B, O],
    correct int64 [S], which is accumulated into (zero it first), and loss fp32
    [S, B] (see _loss_rows), the per-image cross-entropy; with loss the launch is
    dls_lenet5_eval_loss_f32.  O is logits' last dimension, else num_out.  Returns
    (logits, correct)."""
    fn = "lenet5_eval"
    if models.dim() == 1:
        models = models.unsqueeze(0)
    if (models.dtype != torch.float32 or models.dim() != 2 or models.stride(1) != 1
            or (models.shape[0] > 1 and models.stride(0) < models.shape[1])):
        raise RuntimeError(f"{fn}: models must be fp32 [S, ld] rows with unit element stride")
    if (x.dtype != torch.float32 or x.dim() != 4 or tuple(x.shape[1:]) != (1, 32, 32)
            or not x.is_contiguous()):
        raise RuntimeError(f"{fn}: x must be a contiguous fp32 [B, 1, 32, 32] tensor")
    offsets = [int(o) for o in offsets]
    if len(offsets) != 10:
        raise RuntimeError(f"{fn}: ten offsets expected ({', '.join(LENET5_NAMES)})")
    S, B = models.shape[0], x.shape[0]
    if logits is None and correct is None and loss is None:
        raise RuntimeError(f"{fn}: give logits [S, B, O] and / or correct [S]"
                           " and / or loss [S, B]")
    _check_same_device(fn, x, models=models, labels=labels, logits=logits, correct=correct,
                       loss=loss)
    if labels is not None:
        _check_labels(fn, labels, B)
    if correct is not None:
        if labels is None:
            raise RuntimeError(f"{fn}: correct needs labels")
        if (correct.dtype != torch.int64 or tuple(correct.shape) != (S,)
                or not correct.is_contiguous()):
            raise RuntimeError(f"{fn}: correct must be a contiguous int64 [S] tensor")
    if logits is not None:
        if (logits.dtype != torch.float32 or logits.dim() != 3
                or tuple(logits.shape[:2]) != (S, B) or not logits.is_contiguous()):
            raise RuntimeError(f"{fn}: logits must be a contiguous fp32 [S, B, O] tensor")
        if num_out is not None and int(num_out) != logits.shape[2]:
            raise RuntimeError(f"{fn}: num_out={num_out} but logits has {logits.shape[2]} outputs")
        num_out = logits.shape[2]
    elif num_out is None:
        raise RuntimeError(f"{fn}: num_out is needed without logits")
    ldm = _row_pitch(models)
    if loss is not None:
        if labels is None:
            raise RuntimeError(f"{fn}: loss needs labels")
        ldn = _loss_rows(fn, loss, S, B)
        _check(lib().dls_lenet5_eval_loss_f32(_ptr(models), ldm, S, (ctypes.c_int64 * 10)(*offsets),
                                              _ptr(x), B, _ptr(labels), int(num_out), _ptr(logits),
                                              _ptr(correct), _ptr(loss), ldn, _stream(stream, x)),
               "dls_lenet5_eval_loss_f32")
        return logits, correct
    _check(lib().dls_lenet5_eval_f32(_ptr(models), ldm, S, (ctypes.c_int64 * 10)(*offsets),
                                     _ptr(x), B, _ptr(labels), int(num_out), _ptr(logits),
                                     _ptr(correct), _stream(stream, x)), "dls_lenet5_eval_f32")
    return logits, correct


def split_to_f32(x):
    """hi + lo of a split NHWC tensor as fp32 NCHW (test / debugging helper)."""
    c = x.shape[-1] // 2
    u = x.to(torch.int32) & 0xFFFF
    f = (u << 16).view(torch.float32)
    return (f[..., :c] + f[..., c:]).permute(0, 3, 1, 2).contiguous()
