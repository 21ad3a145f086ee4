"""ctypes binding of libnfm_hip.so (the C ABI declared in include/nfm_hip.h).

The shared library is the product: there is NO fallback.  If it is missing, or a
tensor does not live on a ROCm device, the call fails loudly.
"""
import ctypes
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
# (kernel experiments load another build of the library: honoured only under NFM_DEBUG, the one variable the
# product reads; the C++ library reads none)
LIB_PATH = (os.environ.get('NFM_HIP_LIB') if os.environ.get('NFM_DEBUG') else None) or os.path.join(_HERE, 'libnfm_hip.so')

F32, F64 = 0, 1
MAT_SYM, MAT_DIAG, MAT_SCAL, MAT_FULL = 0, 1, 2, 3
FLAG_TS_PERTURB = 1
EIG_VECTORS, EIG_FAST = 1, 2                 # flags of nfm_qr_eig_sym
MAT_PIVOTED, INVERT_PIVOTED = 16, 2          # include/nfm_hip.h: NFM_MAT_PIVOTED, NFM_INVERT_PIVOTED
RED_NANSUM, RED_NANMAX, RED_NANMIN, RED_SUM, RED_MAX, RED_MIN, RED_NANCOUNT, RED_NANSUMSQ = range(8)
MAX_DIM = 16
# include/nfm_hip.h: NFM_FUN_*
FUN = {'exp': 0, 'log': 1, 'sqrt': 2, 'rsqrt': 3, 'pow': 4, 'clamp': 5}
# include/nfm_hip.h: NFM_PENCIL_OP_* (the `op` of nfm_sym_pencil_max_order) and NFM_PENCIL_* (the `mode` of nfm_sym_pencil_eig)
PENCIL_OP_FUNM, PENCIL_OP_FUNM_BACKWARD, PENCIL_OP_EIG, PENCIL_OP_DIST_BACKWARD = range(4)
PENCIL_EIG, PENCIL_DIST2, PENCIL_DIST = range(3)
# include/nfm_hip.h: NFM_EIGH_* (the order and the flag of nfm_sym_eigh) and NFM_EIGH_OP_* (the `op` of nfm_sym_eigh_max_order)
EIGH_ORDER = {'ascending': 0, 'descending': 1, 'abs': 2}
EIGH_VECTORS = 4
EIGH_OP_VALUES, EIGH_OP_VECTORS, EIGH_OP_VALUES_BACKWARD, EIGH_OP_BACKWARD = range(4)
# include/nfm_hip.h: NFM_CHOL_* (the `op` of nfm_sym_chol), NFM_CHOL_FACTORED (its flag) and NFM_CHOL_CLASS_* (the
# `op_class` of nfm_sym_chol_max_order)
CHOL_FACTOR, CHOL_LOGDET, CHOL_MAHA, CHOL_MAHA_SQRT, CHOL_LOGPDF = 0, 5, 6, 7, 8
CHOL_APPLY = {'L': 1, 'LT': 2, 'Linv': 3, 'LTinv': 4}
CHOL_FACTORED = 16
CHOL_CLASS_FACTOR, CHOL_CLASS_APPLY, CHOL_CLASS_SCALAR, CHOL_CLASS_BACKWARD = range(4)
# include/nfm_hip.h: NFM_SIMPLEX_*
SX_SOFTMAX, SX_LOG_SOFTMAX, SX_LOGSUMEXP, SX_LOGIT, SX_SOFTMAX_BWD, SX_LOGSUMEXP_BWD, SX_LOG_SOFTMAX_BWD = range(7)
SX_IMPLICIT_IN, SX_IMPLICIT_OUT, SX_MAX_K = 1, 2, 48
# include/nfm_hip.h: NFM_SPECIAL_*
SP_BESSELI, SP_BESSELI_BWD, SP_RATIO, SP_RATIO_BWD, SP_MVDIGAMMA, SP_MVDIGAMMA_BWD = range(6)
SP_MAX_N = 8
SOLVE_LU, SOLVE_CHOL, SOLVE_MAX_DIM = 0, 1, 8    # include/nfm_hip.h: NFM_SOLVE_*
ROWSOLVE_MIN_DIM = 9                             # include/nfm_hip.h: NFM_ROWSOLVE_MIN_DIM; nfm_rowsolve serves 9..MAX_DIM
SVD_PLAIN, SVD_PINV, SVD_MAX_DIM, SVD_MAX_SWEEPS = 0, 1, 8, 16    # include/nfm_hip.h: NFM_SVD_*
POLAR_SVDVALS, POLAR_SVD, POLAR_POLAR, POLAR_POLAR_BACKWARD = range(4)    # include/nfm_hip.h: NFM_POLAR_OP_*
LSTSQ_MAX_ROWS, LSTSQ_MAX_N = 4096, 8    # include/nfm_hip.h: NFM_LSTSQ_MAX_ROWS, the N of nfm_lstsq_solve
# include/nfm_hip.h: NFM_RT_*
RT_DCT, RT_DST = 0, 1
RT_NORMS = {'backward': 0, 'forward': 1, 'ortho': 2, 'ortho_scipy': 3}
SIDE = {'left': 0, 'right': 1, 'both': 2}
# include/nfm_hip.h: NFM_QUANTILE_*
QUANTILE_INTERP = {'linear': 0, 'lower': 1, 'higher': 2, 'nearest': 3, 'midpoint': 4}
# include/nfm_hip.h: NFM_STOCH_*
STOCH_MAX_VECS = 8
STOCH_RADEMACHER, STOCH_GAUSSIAN = 0, 1
STOCH_SCALE_NONE, STOCH_SCALE_RSQRT, STOCH_SCALE_RSQRT_OR_DROP = 0, 1, 2


class Operand(ctypes.Structure):
    """struct nfm_operand (include/nfm_hip.h)"""
    _fields_ = [('ptr', ctypes.c_void_p),
                ('stride_outer', ctypes.c_int64),
                ('stride_inner', ctypes.c_int64),
                ('stride_row', ctypes.c_int64),
                ('stride_col', ctypes.c_int64)]


_i, _i64, _vp, _op = ctypes.c_int, ctypes.c_int64, ctypes.c_void_p, ctypes.POINTER(Operand)
_dp = ctypes.POINTER(ctypes.c_double)

# name -> argtypes; every symbol include/nfm_hip.h declares
SIGNATURES = {
    'nfm_sym_solve': [_i, _i, _i, _i64, _i64, _op, _op, _op, _dp, _vp],
    'nfm_sym_matvec': [_i, _i, _i, _i, _i64, _i64, _op, _op, _op, _op, _vp],
    'nfm_sym_invert': [_i, _i, _i, _i64, _i64, _op, _op, _vp],
    'nfm_sym_det': [_i, _i, _i64, _i64, _op, _op, _vp],
    'nfm_sym_to_full': [_i, _i, _i64, _i64, _op, _op, _vp],
    'nfm_sym_outer': [_i, _i, _i64, _i64, _op, _op, _vp],
    'nfm_sym_outer2': [_i, _i, _i, _i64, _i64, _op, _op, _op, _vp],
    'nfm_sym_matmul': [_i, _i, _i, _i, _i64, _i64, _op, _op, _op, _vp],
    'nfm_sym_matmul_solve': [_i, _i, _i, _i, _i64, _i64, _op, _op, _op, _op, _dp, _vp],
    # (their `const nfm_operand *` arguments are bound as plain pointers: `byref(Operand)` passes through either, and
    # the frozen table of tests/test_abi_sweep_host.py, the answers of a library that predates these two, lists every
    # entry whose binding names `_op`; tests/test_symfun_host.py sweeps these two with the same canonical bad calls)
    'nfm_sym_funm': [_i, _i, _i, ctypes.c_double, _i, ctypes.c_double, _i64, _i64, _vp, _vp, _vp],
    'nfm_sym_funm_backward': [_i, _i, _i, ctypes.c_double, _i, ctypes.c_double, _i64, _i64, _vp, _vp, _vp, _vp],
    'nfm_sym_funm_max_order': [_i, _i],
    'nfm_sym_funm_host_eval': [_i, _i, ctypes.c_double, _i, ctypes.c_double, _i, _vp, _vp, _vp],
    # (plain pointers as above; tests/test_sympencil_host.py makes the canonical bad calls)
    'nfm_sym_pencil_funm': [_i, _i, _i, ctypes.c_double, _i, ctypes.c_double, _i64, _i64, _vp, _vp, _vp, _vp],
    'nfm_sym_pencil_funm_backward': [_i, _i, _i, ctypes.c_double, _i, ctypes.c_double, _i64, _i64,
                                     _vp, _vp, _vp, _vp, _vp],
    'nfm_sym_pencil_eig': [_i, _i, _i, _i64, _i64, _vp, _vp, _vp, _vp],
    'nfm_sym_pencil_dist_backward': [_i, _i, _i, _i64, _i64, _vp, _vp, _vp, _vp, _vp],
    'nfm_sym_pencil_max_order': [_i, _i],
    # (plain pointers for the same reason as nfm_sym_funm above; tests/test_symeig_host.py makes the canonical bad calls)
    'nfm_sym_eigh': [_i, _i, _i, _i64, _i64, _vp, _vp, _vp],
    'nfm_sym_eigh_backward': [_i, _i, _i, _i64, _i64, _vp, _vp, _vp, _vp, _vp],
    'nfm_sym_eigh_max_order': [_i, _i],
    'nfm_sym_eigh_host_finish': [_i, _i, _i, _i64, _vp, _vp, _vp],
    # (plain pointers for the same reason as nfm_sym_funm above; tests/test_symchol_host.py makes the canonical bad calls)
    'nfm_sym_chol': [_i, _i, _i, _i64, _i64, _vp, _vp, _vp, _vp],
    'nfm_sym_chol_backward': [_i, _i, _i, _i64, _i64, _vp, _vp, _vp, _vp, _vp],
    'nfm_sym_chol_max_order': [_i, _i],
    'nfm_sym_chol_host': [_i, _i, _i, _i64, _vp, _vp, _vp, _vp],
    # (the same; tests/test_cholgrad_host.py makes the canonical bad calls)
    'nfm_sym_chol_grad': [_i, _i, _i, _i64, _i64, _vp, _vp, _vp, _vp, _vp],
    'nfm_sym_chol_grad_max_order': [_i, _i],
    'nfm_sym_chol_grad_host': [_i, _i, _i, _i64, _vp, _vp, _vp, _vp],
    'nfm_batch_inv': [_i, _i, _i, _i64, _i64, _op, _op, _vp],
    'nfm_batch_det': [_i, _i, _i64, _i64, _op, _op, _vp],
    'nfm_batch_matvec': [_i, _i, _i, _i64, _i64, _op, _op, _op, _vp],
    # (plain pointers for the same reason as nfm_sym_funm above; tests/test_polar_host.py makes the canonical bad calls)
    'nfm_batch_svdvals': [_i, _i, _i64, _i64, _vp, _vp, _vp],
    'nfm_batch_svd': [_i, _i, _i64, _i64, _vp, _vp, _vp],
    'nfm_batch_polar': [_i, _i, _i64, _i64, _vp, _vp, _vp],
    'nfm_batch_polar_backward': [_i, _i, _i64, _i64, _vp, _vp, _vp, _vp, _vp],
    'nfm_polar_max_order': [_i, _i],
    'nfm_polar_host': [_i, _i, _i, _i64, _vp, _vp, _vp, _vp],
    'nfm_lie_expm': [_i, _i, _i, ctypes.c_double, _i64, _i64, _op, _op, _vp],
    'nfm_lie_expm_frechet': [_i, _i, _i, ctypes.c_double, _i64, _i64, _op, _op, _op, _op, _vp],
    'nfm_lie_logm': [_i, _i, _i64, _i64, _op, _op, _vp],
    'nfm_lie_logm_solve': [_i, _i, _i64, _i64, _op, _op, _op, _vp],
    'nfm_lie_logm_frechet': [_i, _i, _i64, _i64, _op, _op, _op, _vp],
    'nfm_simplex_forward': [_i, _i, _i, _i, _i64, _i64, _i64, _vp, _vp, _vp, _vp],
    'nfm_simplex_backward': [_i, _i, _i, _i, _i64, _i64, _i64, _vp, _vp, _vp, _vp],
    'nfm_special_besseli': [_i, _i, ctypes.c_double, _i64, _vp, _vp, _vp],
    'nfm_special_besseli_backward': [_i, _i, ctypes.c_double, _i64, _vp, _vp, _vp, _vp, _vp],
    'nfm_special_besseli_ratio': [_i, ctypes.c_double, _i, _i, _i64, _vp, _vp, _vp],
    'nfm_special_besseli_ratio_backward': [_i, ctypes.c_double, _i64, _vp, _vp, _vp, _vp, _vp],
    'nfm_special_mvdigamma': [_i, _i, _i64, _vp, _vp, _vp],
    'nfm_special_mvdigamma_backward': [_i, _i, _i64, _vp, _vp, _vp, _vp],
    'nfm_special_host_eval': [_i, _i, _i, ctypes.c_double, _i, _i, _i64, _vp, _vp, _vp, _vp],
    'nfm_sugar_solve': [_i, _i, _i, _i, _i64, _i64] + 3 * [_vp, _i64, _i64, _i64, _i64] + [_vp],
    'nfm_sugar_max_cols': [_i, _i],
    'nfm_rowsolve': [_i, _i, _i, _i, _i64, _i64] + 3 * [_vp, _i64, _i64, _i64, _i64] + [_vp],
    'nfm_rowsolve_max_cols': [_i, _i],
    'nfm_svd_solve': [_i, _i, _i, _i, _i, ctypes.c_double, _i64, _i64] + 3 * [_vp, _i64, _i64, _i64, _i64] + [_vp],
    'nfm_svd_solve_host': [_i, _i, _i, _i, _i, ctypes.c_double, _i64, _i64] + 3 * [_vp, _i64, _i64, _i64, _i64],
    'nfm_svd_max_cols': [_i, _i, _i],
    'nfm_lstsq_solve': [_i, _i, _i, _i, ctypes.c_double, _i64, _i64] + 3 * [_vp, _i64, _i64, _i64, _i64] + [_vp],
    'nfm_lstsq_solve_host': [_i, _i, _i, _i, ctypes.c_double, _i64, _i64] + 3 * [_vp, _i64, _i64, _i64, _i64],
    'nfm_lstsq_max_cols': [_i, _i],
    'nfm_rt_transform': [_i, _i, _i, _i, _i, _i64, _i64, _i64, _vp, _vp, _vp],
    'nfm_rt_transform_host': [_i, _i, _i, _i, _i, _i64, _i64, _i64, _vp, _vp],
    'nfm_rt_max_len': [_i],
    'nfm_rt_transform_mm': [_i, _i, _i, _i, _i, _i64, _i64, _i64, _vp, _vp, _vp],
    'nfm_rt_mm_max_len': [_i],
    'nfm_reduce_all': [_i, _i, _i, _i64, _vp, _vp, ctypes.c_size_t, _vp, _vp],
    'nfm_reduce_dim_workspace_bytes': [_i, _i, _i64, _i64, _i64, _i],
    'nfm_reduce_dim': [_i, _i, _i, _i64, _i64, _i64, _vp, _vp, ctypes.c_size_t, _vp, _vp, _vp],
    'nfm_reduce_moments_workspace_bytes': [_i, _i64, _i64, _i64],
    'nfm_reduce_moments': [_i, _i64, _i64, _i64, _vp, _vp, ctypes.c_size_t, _vp, _vp],
    'nfm_reduce_stat': [_i, _i, _i, _i64, _i64, _i64, _vp, _vp, ctypes.c_size_t, _vp, _vp],
    'nfm_reduce_median_workspace_bytes': [_i64, _i64],
    'nfm_reduce_median': [_i, _i, _i64, _i64, _vp, _vp, ctypes.c_size_t, _vp, _vp, _vp],
    'nfm_reduce_median_lane_max': [_i],
    'nfm_reduce_median_mid': [_i, _i, _i64, _i64, _i64, _vp, _vp, _vp, _vp],
    'nfm_reduce_quantile_max_q': [],
    'nfm_reduce_quantile_workspace_bytes': [_i64, _i64, _i],
    'nfm_reduce_quantile': [_i, _i, _i, _i64, _i64, _i, _dp, _vp, _vp, ctypes.c_size_t, _vp, _vp, _vp],
    'nfm_reduce_quantile_plan_host': [ctypes.c_double, ctypes.c_uint64, _i, ctypes.POINTER(ctypes.c_uint64),
                                      ctypes.POINTER(ctypes.c_uint64), _dp],
    'nfm_stoch_philox_host': [_vp, _vp, _vp],
    'nfm_stoch_fill': [_i, _i, ctypes.c_uint64, _i64, _i64, _vp, _vp],
    'nfm_stoch_gram_workspace_bytes': [_i, _i],
    'nfm_stoch_gram': [_i, _i, _i, _i64, _vp, _vp, _vp, ctypes.c_size_t, _vp, _i, _vp],
    'nfm_stoch_combine': [_i, _i, _i, _i64, _vp, _vp, _vp, _vp, _i, _vp, _vp, _vp],
    'nfm_qr_givens': [_i, _i64, _i64, _op, _op, _vp, _vp],
    'nfm_qr_givens_apply': [_i, _i, _i, _i, _i, _i64, _i64, _op, _op, _op, _vp],
    'nfm_qr_householder': [_i, _i, _i, _i64, _i64, _op, _vp, _vp],
    'nfm_qr_householder_apply': [_i, _i, _i, _i, _i64, _i64, _op, _op, _vp],
    'nfm_qr_hessenberg': [_i, _i, _i, _i, _i, _i64, _i64, _op, _vp, _vp],
    'nfm_qr_qr_hessenberg': [_i, _i, _i64, _i64, _op, _vp, _vp],
    'nfm_qr_rq_hessenberg': [_i, _i, _i, _i64, _i64, _op, _op, _vp, _vp],
    'nfm_qr_eig_sym': [_i, _i, _i, _i, _i, ctypes.c_double, _i64, _i64, _op, _vp, _vp],
}

_lib = None


def lib():
    """Load the HIP backend; raises if it has not been built (no fallback)."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise ImportError(
                f'nitorch_fastmath_amd: {LIB_PATH} is missing. Build it with '
                '`python -c "import __graft_entry__ as g; g.build()"` or '
                '`make -C nitorch_fastmath_amd/csrc`. There is no CPU fallback.')
        L = ctypes.CDLL(LIB_PATH)
        for name, argtypes in SIGNATURES.items():
            fn = getattr(L, name)
            fn.argtypes = argtypes
            fn.restype = ctypes.c_size_t if name.endswith('_workspace_bytes') else ctypes.c_int
        L.nfm_strerror.argtypes = [ctypes.c_int]
        L.nfm_strerror.restype = ctypes.c_char_p
        L.nfm_version.argtypes = []
        L.nfm_version.restype = ctypes.c_int
        L.nfm_reduce_workspace_bytes.argtypes = []
        L.nfm_reduce_workspace_bytes.restype = ctypes.c_size_t
        _lib = L
    return _lib


def check(rc):
    """C-ABI status -> Python exception (errors never cross the boundary as C++ throws)."""
    if rc == 0:
        return
    msg = lib().nfm_strerror(rc).decode()
    if rc < 0:
        raise ValueError(f'nitorch_fastmath_amd: {msg} (code {rc})')
    raise RuntimeError(f'nitorch_fastmath_amd: HIP error {rc}: {msg}')
