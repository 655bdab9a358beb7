"""tests/gpu_unit/libhb_primitives.so — the device unit wrappers of tests/gpu_unit/primitives.hip (one kernel per device-only primitive
of hb_math.hpp / hb_tile.hpp / hb_qpfactor.hpp) — and one Python face for it and for its host twin (the emu_prim_* exports of
libhostemu.so, same cases through the host branches of the headers).  csrc/build.sh builds the library with the product; build() here
rebuilds it on demand when it is missing or older than a source it includes: one build under a file lock, installed atomically, like
tests/_hostemu.py."""
import ctypes as C
import fcntl
import os
import subprocess
from pathlib import Path

import numpy as np

HERE = Path(__file__).resolve().parent / "gpu_unit"
CSRC = Path(__file__).resolve().parents[1] / "hunter_bipedal_control_amd" / "csrc"

MATH_OPS = {"rcp_t": 0, "ric_rcp": 1, "sincos_reduced": 2, "sincos_t": 3, "sincos_bounded": 4, "log_fd": 5, "rsqrt_t": 6, "sqrt_t": 7,
            "dual_sincos_t": 10, "dual_div": 11, "dual_rcp_t": 12, "dual_sqrt_t": 13}
LANE_OPS = {"wave_max_f64": 0, "wave_max_nonneg_f64": 1, "wave_sum_f64": 2, "quad_sum_f64": 3, "seg8_allsum": 4, "seg8_allmax": 5,
            "wave_bcast_f64": 6, "wave_gather_f64": 7, "seg8_get": 8, "seg8_suffix_sum": 9, "seg8_prefix_sum": 10, "seg8_prefix_product": 11,
            "wave_max_pos_f64": 12}
RT_OPS = {"tile_init": 0, "tile_init_rm": 1, "tile_init_col": 2, "tile_set_col": 3, "tile_add": 4, "tile_store_pre": 5, "tile_store_rm_cols": 6}
TILE_DESC_FIELDS = ("K", "LDA", "TA", "LDB", "TB", "KR", "PRE", "MT", "NT", "WK", "MTB", "NTB")


def build() -> Path:
    so = HERE / "libhb_primitives.so"
    deps = [HERE / "primitives.hip", HERE / "prim_cases.hpp", CSRC / "hipcc_flags.sh", *CSRC.glob("*.hpp")]
    with open(HERE / ".gpuunit.lock", "w") as lock:
        fcntl.flock(lock, fcntl.LOCK_EX)
        if not so.exists() or so.stat().st_mtime < max(d.stat().st_mtime for d in deps):
            hipcc, flags = subprocess.check_output(["bash", "-c", '. "$0"; echo "$HIPCC"; echo "$HB_HIPCC_FLAGS"', str(CSRC / "hipcc_flags.sh")],
                                                   text=True).splitlines()[:2]
            tmp = HERE / f"libhb_primitives.{os.getpid()}.so"
            subprocess.check_call([hipcc, *flags.split(), "-shared", "-o", str(tmp), str(HERE / "primitives.hip")])
            os.replace(tmp, so)
    return so


def _dp(a):
    return a.ctypes.data_as(C.POINTER(C.c_double))


def _ip(a):
    return a.ctypes.data_as(C.POINTER(C.c_int32))


def _f64(a, shape=None):
    a = np.ascontiguousarray(a, dtype=np.float64)
    assert shape is None or a.shape == tuple(shape), (a.shape, shape)
    return a


def _i32(a, shape=None):
    a = np.ascontiguousarray(a, dtype=np.int32)
    assert shape is None or a.shape == tuple(shape), (a.shape, shape)
    return a


_cache = {}


class Prims:
    """The entries of one of the two libraries (prefix "hbp_": device, "emu_prim_": host twin).  Every call checks the int32 status."""

    def __init__(self, lib, prefix):
        self.lib, self.prefix = lib, prefix
        self.on_device = prefix == "hbp_"
        s = np.zeros(8, np.int32)
        self._call("sizes", _ip(s))
        self.n_tile_specs, self.TILE_LDS, self.TILE_DST, self.RT_LD, self.RT_LDD, self.RT_WORDS, self.QF_A, self.QF_R = (int(v) for v in s)

    def _call(self, name, *args):
        # a HIP error (status > 0) is remembered: after a fault nothing more is started on the device by this process
        assert not (self.on_device and _cache.get("hip_error")), f"{self.prefix}{name} not run: {_cache['hip_error']}"
        f = getattr(self.lib, self.prefix + name)
        f.restype = C.c_int32
        st = f(*args)
        if st > 0 and self.on_device:
            _cache["hip_error"] = f"{self.prefix}{name} returned hipError_t {st} earlier"
        assert st == 0, f"{self.prefix}{name}: status {st}"

    def math(self, op, *rows):
        """op over n points; rows: up to four operand arrays of length n -> [4][n] outputs"""
        n = len(rows[0])
        x = np.zeros((4, n))
        for i, r in enumerate(rows):
            x[i] = r
        y = np.full((4, n), np.nan)
        self._call("math", C.c_int32(MATH_OPS[op]), _dp(x), C.c_int32(n), _dp(y))
        return y

    def lanes(self, op, data, idx=None):
        """data: [ncases][words] (words = 64, or 576 for the scans and the prefix product); idx: [ncases][64]"""
        assert self.on_device, "the lane primitives have no host form"
        data = _f64(data)
        ncases, words = data.shape
        idx = np.zeros((ncases, 64), np.int32) if idx is None else _i32(idx, (ncases, 64))
        out = np.full_like(data, np.nan)
        self._call("lanes", C.c_int32(LANE_OPS[op]), C.c_int32(ncases), C.c_int32(words), _dp(data), _ip(idx), _dp(out))
        return out

    def tile_desc(self, tid):
        d = np.zeros(12, np.int32)
        self._call("tile_desc", C.c_int32(tid), _ip(d))
        return dict(zip(TILE_DESC_FIELDS, (int(v) for v in d)))

    def tile_mma(self, tid, img, par, sw, dst):
        img = _f64(img)
        ncases = img.shape[0]
        img = _f64(img, (ncases, self.TILE_LDS))
        par = _i32(par, (ncases, 8))
        dst = _f64(dst, (ncases, self.TILE_DST)).copy()
        self._call("tile_mma", C.c_int32(tid), C.c_int32(ncases), _dp(img), _ip(par), C.c_double(sw), _dp(dst))
        return dst

    def tile_roundtrip(self, a, b, par, scale, dst):
        a = _f64(a)
        ncases = a.shape[0]
        a, b = _f64(a, (ncases, self.RT_WORDS)), _f64(b, (ncases, self.RT_WORDS))
        par = _i32(par, (ncases, 8))
        dst = _f64(dst, (ncases, self.RT_WORDS)).copy()
        flag = np.full(ncases, -1, np.int32)
        self._call("tile_roundtrip", C.c_int32(ncases), _dp(a), _dp(b), _ip(par), C.c_double(scale), _dp(dst), _ip(flag))
        return dst, flag

    def regularised_factor(self, which, A, b, par, dpar, R, J, g):
        A = _f64(A)
        ncases = A.shape[0]
        A, b = _f64(A, (ncases, self.QF_A)), _f64(b, (ncases, 32))
        par, dpar = _i32(par, (ncases, 8)), _f64(dpar, (ncases, 2))
        R, J, g = _f64(R, (ncases, self.QF_R)).copy(), _f64(J, (ncases, self.QF_R)).copy(), _f64(g, (ncases, 16)).copy()
        diag = np.full((ncases, 64), np.nan)
        self._call("regularised_factor", C.c_int32(which), C.c_int32(ncases), _dp(A), _dp(b), _ip(par), _dp(dpar), _dp(R), _dp(J), _dp(g), _dp(diag))
        return R, J, g, diag

    def givens(self, par, R, J, np_, act, is_active, lam):
        par = _i32(par).copy()
        ncases = par.shape[0]
        R, J = _f64(R, (ncases, self.QF_R)).copy(), _f64(J, (ncases, self.QF_R)).copy()
        np_, lam = _f64(np_, (ncases, 64)).copy(), _f64(lam, (ncases, 64)).copy()
        act, is_active = _i32(act, (ncases, 64)).copy(), _i32(is_active, (ncases, 64)).copy()
        self._call("givens", C.c_int32(ncases), _ip(par), _dp(R), _dp(J), _dp(np_), _ip(act), _ip(is_active), _dp(lam))
        return par, R, J, np_, act, is_active, lam


def device() -> Prims:
    if "dev" not in _cache:
        _cache["dev"] = Prims(C.CDLL(str(build())), "hbp_")
    return _cache["dev"]


def host() -> Prims:
    if "host" not in _cache:
        import _hostemu
        _cache["host"] = Prims(C.CDLL(str(_hostemu.build())), "emu_prim_")
    return _cache["host"]
