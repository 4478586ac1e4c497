"""picotls_amd -- MI355X-native AES-GCM record engine for picotls (Python host mirror of the C ABI).

The product is the C ABI in ``include/picotls/mi355x.h`` (``libptls_mi355x.so``: hand-written gfx950 HIP kernels) and
the picotls plugin objects in ``include/picotls/mi355x_picotls.h``. This module binds the same entry points with
ctypes so that Python tests and ``bench.py`` drive exactly the code a C caller would, and mirrors picotls' AEAD
operator interface (``include/picotls.h:519-580, 2082-2164``; ``lib/picotls.c:6547-6601``):

* :data:`aes128gcm` / :data:`aes256gcm` -- algorithm descriptors (``ptls_mi355x_aes{128,256}gcm``)
* :func:`aead_new_direct` / :func:`aead_new` (traffic secret -> key, IV) -> :class:`AeadContext` with ``encrypt`` / ``encrypt_s`` / ``decrypt`` / ``get_iv`` /
  ``set_iv`` / ``xor_iv`` (``decrypt`` returns ``None`` where picotls returns ``SIZE_MAX``)
* :class:`Keyset`, :func:`seal_batch`, :func:`open_batch`, :func:`ecb_batch`, :func:`hp_mask_batch`,
  :func:`seal_batch_hp`, :func:`seal_quic_packets`, :func:`open_quic_packets`, :func:`quiclb_batch` -- the batch
  extension.
* :class:`QuicLbCipher` -- mirror of ``ptls_mi355x_quiclb`` (fusion's ``ptls_fusion_quiclb``).
* :class:`ChaChaKeyset`, :func:`chacha_seal_batch`, :func:`chacha_open_batch`, :func:`chacha_seal_tls_records`,
  :func:`chacha_open_tls_records`, :func:`chacha_hp_mask_batch`, :func:`chacha_seal_quic_packets`,
  :func:`chacha_open_quic_packets`, :data:`chacha20poly1305`, :class:`ChaChaCipher` -- the
  ChaCha20-Poly1305 engine of ``include/picotls/mi355x_chacha20.h`` (``ptls_mi355x_chacha20poly1305`` / ``_chacha20``).

There is no CPU fallback: when the shared object or a gfx950 device is missing every entry point raises.
"""
from __future__ import annotations

import ctypes
import os
from dataclasses import dataclass

import numpy as np

from .records import (CID_DTYPE, HP_DTYPE, QUIC_BAD_MAC, QUIC_KEY_PHASE, QUIC_OK, QUIC_REJECTED, QUIC_RESULT_DTYPE, QUICLB_MAX_LEN,  # noqa: F401
                      QUICLB_MIN_LEN, RECORD_DTYPE, TLS_BAD_HEADER, TLS_BAD_MAC, TLS_OK, TLS_RESULT_DTYPE, TLS_UNEXPECTED_MESSAGE,
                      RecordBatch, shard_ranges)

_PKG = os.path.dirname(os.path.abspath(__file__))
# PTLS_MI355X_LIB: another build of the same engine (an A/B variant under tools/variants/) for the GPU suite
_DEFAULT_LIB = os.path.join(_PKG, "_lib", "libptls_mi355x.so")
LIB_PATH = os.environ.get("PTLS_MI355X_LIB") or _DEFAULT_LIB
PICOTLS_LIB_PATH = os.path.join(_PKG, "_lib", "libptls_mi355x_picotls.so")

# every function of include/picotls/mi355x.h (tests check the .so exports exactly these)
ABI_FUNCTIONS = (
    "ptls_mi355x_is_supported",
    "ptls_mi355x_keyset_new",
    "ptls_mi355x_keyset_free",
    "ptls_mi355x_keyset_size",
    "ptls_mi355x_keyset_key_size",
    "ptls_mi355x_keyset_device",
    "ptls_mi355x_keyset_get_iv",
    "ptls_mi355x_keyset_set_iv",
    "ptls_mi355x_keyset_update",
    "ptls_mi355x_keyset_set_schedule",
    "ptls_mi355x_keyset_set_lane_framed",
    "ptls_mi355x_keyset_get_lane_framed",
    "ptls_mi355x_keyset_set_constant_time",
    "ptls_mi355x_keyset_get_constant_time",
    "ptls_mi355x_seal_batch",
    "ptls_mi355x_open_batch",
    "ptls_mi355x_seal_tls_records",
    "ptls_mi355x_open_tls_records",
    "ptls_mi355x_seal_tls12_records",
    "ptls_mi355x_open_tls12_records",
    "ptls_mi355x_ecb_batch",
    "ptls_mi355x_hp_mask_batch",
    "ptls_mi355x_seal_batch_hp",
    "ptls_mi355x_quiclb_batch",
    "ptls_mi355x_quiclb_transform",
    "ptls_mi355x_encrypt",
    "ptls_mi355x_encrypt_v",
    "ptls_mi355x_encrypt_s",
    "ptls_mi355x_decrypt",
    "ptls_mi355x_encrypt_block",
    "ptls_mi355x_encrypt_blocks",
    "ptls_mi355x_staging_bytes",
    "ptls_mi355x_release_staging",
    "ptls_mi355x_last_error",
)
# every function of include/picotls/mi355x_quic.h: QUIC packet protection under AES-GCM (same shared object)
QUIC_ABI_FUNCTIONS = (
    "ptls_mi355x_seal_quic_packets",
    "ptls_mi355x_open_quic_packets",
)
# include/picotls/mi355x_debug.h: test and measurement hooks (not the picotls boundary)
DEBUG_FUNCTIONS = (
    "ptls_mi355x_debug_counters",
    "ptls_mi355x_debug_inject_error",
    "ptls_mi355x_debug_clock_sample",
    "ptls_mi355x_debug_wallclock_khz",
    "ptls_mi355x_debug_kernel_clock",
    "ptls_mi355x_debug_kernel_clock_count",
)

# every function of include/picotls/mi355x_chacha20.h: the ChaCha20-Poly1305 engine (same shared object)
CHACHA_ABI_FUNCTIONS = (
    "ptls_mi355x_chacha_keyset_new",
    "ptls_mi355x_chacha_keyset_free",
    "ptls_mi355x_chacha_keyset_size",
    "ptls_mi355x_chacha_keyset_device",
    "ptls_mi355x_chacha_keyset_update",
    "ptls_mi355x_chacha_keyset_get_iv",
    "ptls_mi355x_chacha_keyset_set_iv",
    "ptls_mi355x_chacha_seal_batch",
    "ptls_mi355x_chacha_open_batch",
    "ptls_mi355x_chacha_seal_tls_records",
    "ptls_mi355x_chacha_open_tls_records",
    "ptls_mi355x_chacha_hp_mask_batch",
    "ptls_mi355x_chacha_seal_quic_packets",
    "ptls_mi355x_chacha_open_quic_packets",
    "ptls_mi355x_chacha_encrypt",
    "ptls_mi355x_chacha_encrypt_v",
    "ptls_mi355x_chacha_decrypt",
    "ptls_mi355x_chacha_hp_mask",
    "ptls_mi355x_chacha_debug_poly1305",
    "ptls_mi355x_chacha_debug_force",
    "ptls_mi355x_chacha_debug_counters",
    "ptls_mi355x_chacha_debug_spread",
    "ptls_mi355x_chacha_debug_spread_counters",
    "ptls_mi355x_chacha_debug_spread_params",
    "ptls_mi355x_chacha_debug_rpow",
)

SIZE_MAX = ctypes.c_size_t(-1).value
_lib = None


class EngineError(RuntimeError):
    pass


def load_library(path: str = LIB_PATH) -> ctypes.CDLL:
    """Loads libptls_mi355x.so (no device calls). Raises if it was not built."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(path):
        raise EngineError(f"{path} is missing: run `python -c 'import __graft_entry__ as g; g.build()'` "
                          "(hipcc --offload-arch=gfx950); there is no CPU fallback")
    if path == _DEFAULT_LIB:  # the in-tree build must be of the sources beside it (build.py's digest stamp)
        from . import build as _b

        if os.path.exists(_b.ENGINE_SRCS[0]) and _b._stamp(path) != _b.engine_digest():
            raise EngineError(f"{path} was not built from the current sources (its {path}.sha256 differs): rebuild with "
                              "`python -c 'import __graft_entry__ as g; g.build()'`")
    lib = ctypes.CDLL(path)
    vp, sz, u64, ci = ctypes.c_void_p, ctypes.c_size_t, ctypes.c_uint64, ctypes.c_int
    lib.ptls_mi355x_is_supported.restype = ci
    lib.ptls_mi355x_keyset_new.argtypes = [vp, vp, sz, sz]
    lib.ptls_mi355x_keyset_new.restype = vp
    lib.ptls_mi355x_keyset_free.argtypes = [vp]
    lib.ptls_mi355x_keyset_size.argtypes = [vp]
    lib.ptls_mi355x_keyset_size.restype = sz
    lib.ptls_mi355x_keyset_key_size.argtypes = [vp]
    lib.ptls_mi355x_keyset_key_size.restype = sz
    lib.ptls_mi355x_keyset_device.argtypes = [vp]
    lib.ptls_mi355x_keyset_device.restype = ci
    lib.ptls_mi355x_staging_bytes.restype = sz
    lib.ptls_mi355x_release_staging.restype = None
    lib.ptls_mi355x_keyset_get_iv.argtypes = [vp, sz, vp]
    lib.ptls_mi355x_keyset_set_iv.argtypes = [vp, sz, vp]
    lib.ptls_mi355x_keyset_update.argtypes = [vp, vp, vp, vp, sz]
    lib.ptls_mi355x_keyset_set_schedule.argtypes = [vp, ci]
    lib.ptls_mi355x_keyset_set_lane_framed.argtypes = [vp, ci]
    lib.ptls_mi355x_keyset_get_lane_framed.argtypes = [vp]
    lib.ptls_mi355x_keyset_get_lane_framed.restype = ci
    lib.ptls_mi355x_keyset_set_constant_time.argtypes = [vp, ci]
    lib.ptls_mi355x_keyset_get_constant_time.argtypes = [vp]
    lib.ptls_mi355x_keyset_get_constant_time.restype = ci
    lib.ptls_mi355x_seal_batch.argtypes = [vp, vp, sz, vp, vp, vp, vp]
    lib.ptls_mi355x_open_batch.argtypes = [vp, vp, sz, vp, vp, vp, vp, vp]
    lib.ptls_mi355x_ecb_batch.argtypes = [vp, vp, vp, vp, sz, vp]
    lib.ptls_mi355x_hp_mask_batch.argtypes = [vp, vp, sz, vp, vp, vp]
    lib.ptls_mi355x_seal_tls_records.argtypes = [vp, vp, sz, vp, vp, vp]
    lib.ptls_mi355x_open_tls_records.argtypes = [vp, vp, sz, vp, vp, vp, vp, vp]
    lib.ptls_mi355x_seal_tls12_records.argtypes = [vp, vp, sz, vp, vp, vp]
    lib.ptls_mi355x_open_tls12_records.argtypes = [vp, vp, sz, vp, vp, vp, vp, vp]
    lib.ptls_mi355x_seal_batch_hp.argtypes = [vp, vp, sz, vp, vp, vp, vp, vp, vp, vp]
    lib.ptls_mi355x_seal_quic_packets.argtypes = [vp, vp, vp, sz, vp, vp, vp]
    lib.ptls_mi355x_open_quic_packets.argtypes = [vp, vp, vp, sz, vp, vp, vp, vp, vp]
    lib.ptls_mi355x_encrypt.argtypes = [vp, sz, vp, vp, sz, u64, vp, sz]
    lib.ptls_mi355x_encrypt_v.argtypes = [vp, sz, vp, vp, sz, u64, vp, sz]
    lib.ptls_mi355x_encrypt_s.argtypes = [vp, sz, vp, vp, sz, u64, vp, sz, vp, sz, sz, vp]
    lib.ptls_mi355x_decrypt.argtypes = [vp, sz, vp, vp, sz, u64, vp, sz]
    lib.ptls_mi355x_decrypt.restype = sz
    lib.ptls_mi355x_encrypt_block.argtypes = [vp, sz, vp, vp]
    lib.ptls_mi355x_encrypt_blocks.argtypes = [vp, sz, vp, vp, sz]
    lib.ptls_mi355x_quiclb_batch.argtypes = [vp, vp, sz, vp, vp, vp]
    lib.ptls_mi355x_quiclb_transform.argtypes = [vp, sz, vp, vp, sz, ci]
    lib.ptls_mi355x_last_error.restype = ctypes.c_char_p
    lib.ptls_mi355x_debug_counters.argtypes = [vp, ci]
    lib.ptls_mi355x_debug_inject_error.restype = ci
    lib.ptls_mi355x_debug_clock_sample.argtypes = [vp, vp]
    lib.ptls_mi355x_debug_wallclock_khz.restype = ci
    lib.ptls_mi355x_debug_kernel_clock.argtypes = [vp, ctypes.c_uint]
    lib.ptls_mi355x_debug_kernel_clock_count.restype = ci
    lib.ptls_mi355x_chacha_keyset_new.argtypes = [vp, vp, sz]
    lib.ptls_mi355x_chacha_keyset_new.restype = vp
    lib.ptls_mi355x_chacha_keyset_free.argtypes = [vp]
    lib.ptls_mi355x_chacha_keyset_free.restype = None
    lib.ptls_mi355x_chacha_keyset_size.argtypes = [vp]
    lib.ptls_mi355x_chacha_keyset_size.restype = sz
    lib.ptls_mi355x_chacha_keyset_device.argtypes = [vp]
    lib.ptls_mi355x_chacha_keyset_device.restype = ci
    lib.ptls_mi355x_chacha_keyset_update.argtypes = [vp, vp, vp, vp, sz]
    lib.ptls_mi355x_chacha_keyset_get_iv.argtypes = [vp, sz, vp]
    lib.ptls_mi355x_chacha_keyset_set_iv.argtypes = [vp, sz, vp]
    lib.ptls_mi355x_chacha_seal_batch.argtypes = [vp, vp, sz, vp, vp, vp, vp]
    lib.ptls_mi355x_chacha_open_batch.argtypes = [vp, vp, sz, vp, vp, vp, vp, vp]
    lib.ptls_mi355x_chacha_seal_tls_records.argtypes = [vp, vp, sz, vp, vp, vp]
    lib.ptls_mi355x_chacha_open_tls_records.argtypes = [vp, vp, sz, vp, vp, vp, vp, vp]
    lib.ptls_mi355x_chacha_hp_mask_batch.argtypes = [vp, vp, sz, vp, vp, vp]
    lib.ptls_mi355x_chacha_seal_quic_packets.argtypes = [vp, vp, vp, sz, vp, vp, vp]
    lib.ptls_mi355x_chacha_open_quic_packets.argtypes = [vp, vp, vp, sz, vp, vp, vp, vp, vp]
    lib.ptls_mi355x_chacha_encrypt.argtypes = [vp, sz, vp, vp, sz, u64, vp, sz]
    lib.ptls_mi355x_chacha_encrypt_v.argtypes = [vp, sz, vp, vp, sz, u64, vp, sz]
    lib.ptls_mi355x_chacha_decrypt.argtypes = [vp, sz, vp, vp, sz, u64, vp, sz]
    lib.ptls_mi355x_chacha_decrypt.restype = sz
    lib.ptls_mi355x_chacha_hp_mask.argtypes = [vp, sz, vp, vp]
    lib.ptls_mi355x_chacha_debug_poly1305.argtypes = [vp, vp, sz, vp]
    lib.ptls_mi355x_chacha_debug_force.argtypes = [ci, ci]
    lib.ptls_mi355x_chacha_debug_counters.argtypes = [vp, ci]
    lib.ptls_mi355x_chacha_debug_spread.argtypes = [ci, ci, ci]
    lib.ptls_mi355x_chacha_debug_spread_counters.argtypes = [vp, ci]
    lib.ptls_mi355x_chacha_debug_spread_params.argtypes = [vp]
    lib.ptls_mi355x_chacha_debug_rpow.argtypes = [vp, u64, vp]
    _lib = lib
    return lib


def _err(what: str) -> EngineError:
    msg = load_library().ptls_mi355x_last_error()
    return EngineError(f"{what}: {msg.decode() if msg else 'unknown error'}")


def is_supported() -> bool:
    return bool(load_library().ptls_mi355x_is_supported())


def _buf(b) -> ctypes.c_void_p | None:
    if b is None or len(b) == 0:
        return None
    if isinstance(b, bytes):
        return ctypes.cast(ctypes.c_char_p(b), ctypes.c_void_p)
    if isinstance(b, bytearray):
        return ctypes.c_void_p(ctypes.addressof((ctypes.c_char * len(b)).from_buffer(b)))
    if isinstance(b, np.ndarray):
        return ctypes.c_void_p(b.ctypes.data)
    raise TypeError(type(b))


# ------------------------------------------------------------------------------------------------ keysets / batches


class Keyset:
    """N AES-GCM traffic keys resident on the current device (ptls_mi355x_keyset_new)."""

    def __init__(self, keys: bytes | np.ndarray, ivs: bytes | np.ndarray, key_size: int):
        lib = load_library()
        keys = np.frombuffer(bytes(keys), dtype=np.uint8) if not isinstance(keys, np.ndarray) else np.ascontiguousarray(keys, np.uint8)
        ivs = np.frombuffer(bytes(ivs), dtype=np.uint8) if not isinstance(ivs, np.ndarray) else np.ascontiguousarray(ivs, np.uint8)
        if key_size not in (16, 32) or keys.size % key_size or ivs.size != keys.size // key_size * 12:
            raise ValueError("keys must be n*key_size bytes and ivs n*12 bytes")
        self.n = keys.size // key_size
        self.key_size = key_size
        h = lib.ptls_mi355x_keyset_new(_buf(keys), _buf(ivs), self.n, key_size)
        if not h:
            raise _err("ptls_mi355x_keyset_new")
        self.handle = ctypes.c_void_p(h)

    def free(self):
        if getattr(self, "handle", None):
            load_library().ptls_mi355x_keyset_free(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass

    def get_iv(self, idx: int = 0) -> bytes:
        out = bytearray(12)
        if load_library().ptls_mi355x_keyset_get_iv(self.handle, idx, _buf(out)) != 0:
            raise _err("get_iv")
        return bytes(out)

    def set_iv(self, iv: bytes, idx: int = 0) -> None:
        if load_library().ptls_mi355x_keyset_set_iv(self.handle, idx, _buf(bytes(iv))) != 0:
            raise _err("set_iv")

    def update(self, key_idx, keys: bytes, ivs: bytes) -> None:
        """Rekeys entries key_idx (ptls_mi355x_keyset_update), e.g. after a TLS 1.3 KeyUpdate."""
        idx = np.ascontiguousarray(key_idx, dtype=np.uint32)
        k = np.frombuffer(bytes(keys), np.uint8)
        v = np.frombuffer(bytes(ivs), np.uint8)
        if k.size != idx.size * self.key_size or v.size != idx.size * 12:
            raise ValueError("keys must be n*key_size bytes and ivs n*12 bytes")
        if load_library().ptls_mi355x_keyset_update(self.handle, _buf(idx), _buf(k), _buf(v), idx.size) != 0:
            raise _err("keyset_update")

    def set_constant_time(self, on: bool = True) -> None:
        """Constant-time GHASH variant (ptls_mi355x_keyset_set_constant_time)."""
        if load_library().ptls_mi355x_keyset_set_constant_time(self.handle, 1 if on else 0) != 0:
            raise _err("set_constant_time")

    @property
    def constant_time(self) -> bool:
        return bool(load_library().ptls_mi355x_keyset_get_constant_time(self.handle))

    SCHEDULES = {"auto": 0, "lockstep": 1, "chunked": 2, "record_per_lane": 3}

    def set_schedule(self, schedule: str, allow_variable_time: bool = False) -> None:
        """Batch schedule (ptls_mi355x_keyset_set_schedule): "auto", "lockstep", "chunked" or "record_per_lane".

        "record_per_lane" (opt-in) runs seal_batch, open_batch and the QUIC packet calls one record per GPU lane, with no
        per-key precomputation and no key order: for large batches of short records over many keys. Records and AADs are
        then limited to PTLS_MI355X_LANE_MAX_LEN (64 KiB) in those calls; every other call runs as under "auto".

        The lockstep schedule (the round-1 kernel, kept for comparison) has data-dependent LDS bank conflicts, so the
        engine never runs it for a constant-time keyset (every keyset is one by default since round 4): the C call
        records the schedule and such a keyset keeps the chunked kernels. Here asking for "lockstep" on a constant-time
        keyset raises, unless allow_variable_time=True, which (after the schedule is set) turns the keyset's
        constant-time setting off so that the lockstep kernel is the one that runs."""
        if schedule not in self.SCHEDULES:
            raise ValueError(f"unknown schedule {schedule!r}")
        lockstep_ct = schedule == "lockstep" and self.constant_time
        if lockstep_ct and not allow_variable_time:
            raise EngineError("set_schedule('lockstep') on a constant-time keyset: the lockstep kernel is not constant-time; "
                              "pass allow_variable_time=True to turn the keyset's constant-time setting off")
        if load_library().ptls_mi355x_keyset_set_schedule(self.handle, self.SCHEDULES[schedule]) != 0:
            raise _err("set_schedule")
        if lockstep_ct:
            self.set_constant_time(False)

    def set_lane_framed(self, on: bool = True) -> None:
        """Under the "record_per_lane" schedule, run the TLS 1.3 and TLS 1.2 framed calls and seal_batch_hp one record
        per GPU lane too (ptls_mi355x_keyset_set_lane_framed). Off on a new keyset; no effect under another schedule;
        survives set_schedule. seal_batch_hp then makes two launches: the lane seal and hp_mask_batch."""
        if load_library().ptls_mi355x_keyset_set_lane_framed(self.handle, 1 if on else 0) != 0:
            raise _err("set_lane_framed")

    @property
    def lane_framed(self) -> bool:
        return bool(load_library().ptls_mi355x_keyset_get_lane_framed(self.handle))


def seal_batch(ks: Keyset, recs_ptr: int, nrecs: int, in_ptr: int, aad_ptr: int, out_ptr: int, stream: int = 0) -> None:
    """Device pointers (ints, e.g. torch ``tensor.data_ptr()``); asynchronous on ``stream`` (a hipStream_t)."""
    if load_library().ptls_mi355x_seal_batch(ks.handle, recs_ptr, nrecs, in_ptr, aad_ptr or None, out_ptr, stream or None) != 0:
        raise _err("ptls_mi355x_seal_batch")


def open_batch(ks: Keyset, recs_ptr: int, nrecs: int, in_ptr: int, aad_ptr: int, out_ptr: int, ok_ptr: int,
               stream: int = 0) -> None:
    if load_library().ptls_mi355x_open_batch(ks.handle, recs_ptr, nrecs, in_ptr, aad_ptr or None, out_ptr, ok_ptr,
                                             stream or None) != 0:
        raise _err("ptls_mi355x_open_batch")


def ecb_batch(ks: Keyset, key_idx_ptr: int, in_ptr: int, out_ptr: int, nblocks: int, stream: int = 0) -> None:
    if load_library().ptls_mi355x_ecb_batch(ks.handle, key_idx_ptr or None, in_ptr, out_ptr, nblocks, stream or None) != 0:
        raise _err("ptls_mi355x_ecb_batch")


def seal_tls_records(ks: Keyset, recs_ptr: int, nrecs: int, in_ptr: int, out_ptr: int, stream: int = 0) -> None:
    """TLS 1.3 wire records (header || ciphertext || tag) from payloads + inner content types (flags); device pointers."""
    if load_library().ptls_mi355x_seal_tls_records(ks.handle, recs_ptr, nrecs, in_ptr, out_ptr, stream or None) != 0:
        raise _err("ptls_mi355x_seal_tls_records")


def open_tls_records(ks: Keyset, recs_ptr: int, nrecs: int, in_ptr: int, out_ptr: int, ok_ptr: int, results_ptr: int = 0,
                     stream: int = 0) -> None:
    """Opens TLS 1.3 wire records and strips the inner type and padding (TLS_RESULT_DTYPE results); device pointers."""
    if load_library().ptls_mi355x_open_tls_records(ks.handle, recs_ptr, nrecs, in_ptr, out_ptr, ok_ptr, results_ptr or None,
                                                   stream or None) != 0:
        raise _err("ptls_mi355x_open_tls_records")


def seal_tls12_records(ks: Keyset, recs_ptr: int, nrecs: int, in_ptr: int, out_ptr: int, stream: int = 0) -> None:
    """TLS 1.2 wire records (header || explicit nonce || ciphertext || tag) from explicit nonce || payload; device pointers."""
    if load_library().ptls_mi355x_seal_tls12_records(ks.handle, recs_ptr, nrecs, in_ptr, out_ptr, stream or None) != 0:
        raise _err("ptls_mi355x_seal_tls12_records")


def open_tls12_records(ks: Keyset, recs_ptr: int, nrecs: int, in_ptr: int, out_ptr: int, ok_ptr: int, results_ptr: int = 0,
                       stream: int = 0) -> None:
    """Opens TLS 1.2 wire records (TLS_RESULT_DTYPE results: content type, length, status); device pointers."""
    if load_library().ptls_mi355x_open_tls12_records(ks.handle, recs_ptr, nrecs, in_ptr, out_ptr, ok_ptr, results_ptr or None,
                                                     stream or None) != 0:
        raise _err("ptls_mi355x_open_tls12_records")


def hp_mask_batch(hp_ks: Keyset, hp_ptr: int, n: int, base_ptr: int, masks_ptr: int, stream: int = 0) -> None:
    """QUIC header-protection masks (HP_DTYPE entries); device pointers."""
    if load_library().ptls_mi355x_hp_mask_batch(hp_ks.handle, hp_ptr, n, base_ptr, masks_ptr, stream or None) != 0:
        raise _err("ptls_mi355x_hp_mask_batch")


def seal_batch_hp(ks: Keyset, recs_ptr: int, nrecs: int, in_ptr: int, aad_ptr: int, out_ptr: int, hp_ks: Keyset,
                  hp_ptr: int, masks_ptr: int, stream: int = 0) -> None:
    """seal_batch followed by the header-protection masks of samples in the sealed output (fusion's supp)."""
    if load_library().ptls_mi355x_seal_batch_hp(ks.handle, recs_ptr, nrecs, in_ptr, aad_ptr or None, out_ptr, hp_ks.handle,
                                                hp_ptr, masks_ptr, stream or None) != 0:
        raise _err("ptls_mi355x_seal_batch_hp")


def _quic_packets(name: str, ks_handle, hp_ks, recs_ptr: int, nrecs: int, in_ptr: int, out_ptr: int, stream: int, *open_ptrs: int) -> None:
    """The C call `name` of the four QUIC packet calls: ks's handle as the caller passes it, hp_ks (None travels as NULL,
    which the engine refuses), and for an open ok and results between out and stream."""
    if getattr(load_library(), name)(ks_handle, hp_ks.handle if hp_ks is not None else None, recs_ptr, nrecs, in_ptr, out_ptr,
                                     *(p or None for p in open_ptrs), stream or None) != 0:
        raise _err(name)


def seal_quic_packets(ks: Keyset, hp_ks: Keyset, recs_ptr: int, nrecs: int, in_ptr: int, out_ptr: int, stream: int = 0) -> None:
    """QUIC packet protection under AES-GCM (RFC 9001 5.3-5.4) in one call: cleartext header || payload at in + in_off
    (aad_len header bytes, len payload bytes, seq the full packet number) to protected header || ciphertext || tag at
    out + out_off, the mask AES-ECB(hp_ks key, sample); device pointers."""
    _quic_packets("ptls_mi355x_seal_quic_packets", ks.handle if ks is not None else None, hp_ks, recs_ptr, nrecs, in_ptr, out_ptr, stream)


def open_quic_packets(ks: Keyset, hp_ks: Keyset, recs_ptr: int, nrecs: int, in_ptr: int, out_ptr: int, ok_ptr: int,
                      results_ptr: int, stream: int = 0) -> None:
    """Removes header protection and opens protected QUIC packets under AES-GCM (aad_len the packet-number offset, len
    the bytes from there to the packet's end, seq the expected packet number, flags bit 0 the expected key phase):
    unprotected header || plaintext to out + out_off, QUIC_RESULT_DTYPE results (both ok and results are required);
    device pointers."""
    _quic_packets("ptls_mi355x_open_quic_packets", ks.handle if ks is not None else None, hp_ks, recs_ptr, nrecs, in_ptr, out_ptr, stream,
                  ok_ptr, results_ptr)


def quiclb_batch(ks: Keyset, cids_ptr: int, n: int, in_ptr: int, out_ptr: int, stream: int = 0) -> None:
    """QUIC-LB CID encryption / decryption (CID_DTYPE entries, AES-128 keyset); device pointers."""
    if load_library().ptls_mi355x_quiclb_batch(ks.handle, cids_ptr, n, in_ptr, out_ptr, stream or None) != 0:
        raise _err("ptls_mi355x_quiclb_batch")


# ------------------------------------------------------------------------------------------------ ChaCha20-Poly1305


class ChaChaKeyset:
    """N ChaCha20-Poly1305 traffic keys (32-byte key, 12-byte static IV) resident on the current device
    (ptls_mi355x_chacha_keyset_new). Sizes are checked before anything touches a device."""

    key_size = 32

    def __init__(self, keys: bytes | np.ndarray, ivs: bytes | np.ndarray):
        keys = np.frombuffer(bytes(keys), dtype=np.uint8) if not isinstance(keys, np.ndarray) else np.ascontiguousarray(keys, np.uint8)
        ivs = np.frombuffer(bytes(ivs), dtype=np.uint8) if not isinstance(ivs, np.ndarray) else np.ascontiguousarray(ivs, np.uint8)
        if keys.size == 0 or keys.size % 32 or ivs.size != keys.size // 32 * 12:
            raise ValueError("keys must be n*32 bytes and ivs n*12 bytes")
        lib = load_library()
        self.n = keys.size // 32
        h = lib.ptls_mi355x_chacha_keyset_new(_buf(keys), _buf(ivs), self.n)
        if not h:
            raise _err("ptls_mi355x_chacha_keyset_new")
        self.handle = ctypes.c_void_p(h)

    def free(self):
        if getattr(self, "handle", None):
            load_library().ptls_mi355x_chacha_keyset_free(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass

    def get_iv(self, idx: int = 0) -> bytes:
        out = bytearray(12)
        if load_library().ptls_mi355x_chacha_keyset_get_iv(self.handle, idx, _buf(out)) != 0:
            raise _err("chacha get_iv")
        return bytes(out)

    def set_iv(self, iv: bytes, idx: int = 0) -> None:
        if len(iv) != 12:
            raise ValueError("the static IV is 12 bytes")
        if load_library().ptls_mi355x_chacha_keyset_set_iv(self.handle, idx, _buf(bytes(iv))) != 0:
            raise _err("chacha set_iv")

    def update(self, key_idx, keys: bytes, ivs: bytes) -> None:
        """Rekeys entries key_idx (ptls_mi355x_chacha_keyset_update), stream-ordered like Keyset.update."""
        idx = np.ascontiguousarray(key_idx, dtype=np.uint32)
        k = np.frombuffer(bytes(keys), np.uint8)
        v = np.frombuffer(bytes(ivs), np.uint8)
        if k.size != idx.size * 32 or v.size != idx.size * 12:
            raise ValueError("keys must be n*32 bytes and ivs n*12 bytes")
        if load_library().ptls_mi355x_chacha_keyset_update(self.handle, _buf(idx), _buf(k), _buf(v), idx.size) != 0:
            raise _err("chacha keyset_update")


def chacha_seal_batch(ks: ChaChaKeyset, recs_ptr: int, nrecs: int, in_ptr: int, aad_ptr: int, out_ptr: int, stream: int = 0) -> None:
    """seal_batch under ChaCha20-Poly1305: device pointers, asynchronous on ``stream``."""
    if load_library().ptls_mi355x_chacha_seal_batch(ks.handle, recs_ptr, nrecs, in_ptr, aad_ptr or None, out_ptr, stream or None) != 0:
        raise _err("ptls_mi355x_chacha_seal_batch")


def chacha_open_batch(ks: ChaChaKeyset, recs_ptr: int, nrecs: int, in_ptr: int, aad_ptr: int, out_ptr: int, ok_ptr: int,
                      stream: int = 0) -> None:
    """open_batch under ChaCha20-Poly1305. A record whose tag fails reports ok = 0; its bytes in ``out`` may have been
    written and must not be used."""
    if load_library().ptls_mi355x_chacha_open_batch(ks.handle, recs_ptr, nrecs, in_ptr, aad_ptr or None, out_ptr, ok_ptr,
                                                    stream or None) != 0:
        raise _err("ptls_mi355x_chacha_open_batch")


def chacha_seal_tls_records(ks: ChaChaKeyset, recs_ptr: int, nrecs: int, in_ptr: int, out_ptr: int, stream: int = 0) -> None:
    """TLS 1.3 wire records under ChaCha20-Poly1305 (layout of seal_tls_records); device pointers."""
    if load_library().ptls_mi355x_chacha_seal_tls_records(ks.handle, recs_ptr, nrecs, in_ptr, out_ptr, stream or None) != 0:
        raise _err("ptls_mi355x_chacha_seal_tls_records")


def chacha_open_tls_records(ks: ChaChaKeyset, recs_ptr: int, nrecs: int, in_ptr: int, out_ptr: int, ok_ptr: int,
                            results_ptr: int = 0, stream: int = 0) -> None:
    """Opens TLS 1.3 wire records under ChaCha20-Poly1305 (TLS_RESULT_DTYPE results); device pointers."""
    if load_library().ptls_mi355x_chacha_open_tls_records(ks.handle, recs_ptr, nrecs, in_ptr, out_ptr, ok_ptr,
                                                          results_ptr or None, stream or None) != 0:
        raise _err("ptls_mi355x_chacha_open_tls_records")


def chacha_hp_mask_batch(hp_ks: ChaChaKeyset, hp_ptr: int, n: int, base_ptr: int, masks_ptr: int, stream: int = 0) -> None:
    """QUIC header-protection masks of the ChaCha20 suites (HP_DTYPE entries, 16 bytes per mask); device pointers."""
    if load_library().ptls_mi355x_chacha_hp_mask_batch(hp_ks.handle, hp_ptr, n, base_ptr, masks_ptr, stream or None) != 0:
        raise _err("ptls_mi355x_chacha_hp_mask_batch")


def chacha_seal_quic_packets(ks: ChaChaKeyset, hp_ks: ChaChaKeyset, recs_ptr: int, nrecs: int, in_ptr: int, out_ptr: int,
                             stream: int = 0) -> None:
    """QUIC packet protection (RFC 9001 5.3-5.4) in one launch: cleartext header || payload at in + in_off (aad_len header
    bytes, len payload bytes, seq the full packet number) to protected header || ciphertext || tag; device pointers."""
    _quic_packets("ptls_mi355x_chacha_seal_quic_packets", ks.handle, hp_ks, recs_ptr, nrecs, in_ptr, out_ptr, stream)


def chacha_open_quic_packets(ks: ChaChaKeyset, hp_ks: ChaChaKeyset, recs_ptr: int, nrecs: int, in_ptr: int, out_ptr: int,
                             ok_ptr: int, results_ptr: int, stream: int = 0) -> None:
    """Removes header protection and opens protected QUIC packets (aad_len the packet-number offset, len the bytes from
    there to the packet's end, seq the expected packet number, flags bit 0 the expected key phase): unprotected header ||
    plaintext to out + out_off, QUIC_RESULT_DTYPE results (both ok and results are required); device pointers."""
    _quic_packets("ptls_mi355x_chacha_open_quic_packets", ks.handle, hp_ks, recs_ptr, nrecs, in_ptr, out_ptr, stream, ok_ptr, results_ptr)


def chacha_debug_poly1305(key32: bytes, msg: bytes) -> bytes:
    """The device Poly1305 routine on a given one-time key (ptls_mi355x_chacha_debug_poly1305)."""
    if len(key32) != 32:
        raise ValueError("the one-time key is 32 bytes")
    tag = bytearray(16)
    if load_library().ptls_mi355x_chacha_debug_poly1305(_buf(bytes(key32)), _buf(bytes(msg)), len(msg), _buf(tag)) != 0:
        raise _err("ptls_mi355x_chacha_debug_poly1305")
    return bytes(tag)


CHACHA_GROUP_WIDTHS = (4, 16)  # lanes per record of the compiled seal / open variants


def chacha_debug_force(group_lanes: int = 0, max_workgroups: int = 0) -> None:
    """0, 0 = automatic; otherwise the group width (one of CHACHA_GROUP_WIDTHS) and a cap on the launch grid."""
    if load_library().ptls_mi355x_chacha_debug_force(group_lanes, max_workgroups) != 0:
        raise _err("ptls_mi355x_chacha_debug_force")


def chacha_debug_counters(reset: bool = False) -> dict:
    """Launches per group width since the last reset: {4: n, 16: n}. Waits for the device."""
    out = (ctypes.c_uint64 * 2)()
    if load_library().ptls_mi355x_chacha_debug_counters(ctypes.cast(out, ctypes.c_void_p), 1 if reset else 0) != 0:
        raise _err("ptls_mi355x_chacha_debug_counters")
    return dict(zip(CHACHA_GROUP_WIDTHS, (int(out[0]), int(out[1]))))


CHACHA_SPREAD_MAX_PIECES = 1024  # PTLS_MI355X_CHACHA_SPREAD_MAX_PIECES: pieces a record is cut into at the most
CHACHA_SPREAD_COUNTERS = ("launches", "pieces", "finished", "whole")


def chacha_debug_spread(piece_bytes: int = 0, min_len: int = 0, force: bool = False) -> None:
    """0, 0, False = automatic; otherwise the base piece length (a multiple of 1024), the length from which a record is
    cut (batches and per-record calls alike) and whether a forced group width still lets a launch spread."""
    if load_library().ptls_mi355x_chacha_debug_spread(piece_bytes, min_len, 1 if force else 0) != 0:
        raise _err("ptls_mi355x_chacha_debug_spread")


def chacha_debug_spread_counters(reset: bool = False) -> dict:
    """Since the last reset: spread launches, pieces run, records finished by a combine, whole records run in spread
    launches (CHACHA_SPREAD_COUNTERS). Waits for the device."""
    out = (ctypes.c_uint64 * 4)()
    if load_library().ptls_mi355x_chacha_debug_spread_counters(ctypes.cast(out, ctypes.c_void_p), 1 if reset else 0) != 0:
        raise _err("ptls_mi355x_chacha_debug_spread_counters")
    return dict(zip(CHACHA_SPREAD_COUNTERS, (int(x) for x in out)))


def chacha_debug_spread_params() -> dict:
    """The compiled tunables: min_batch / min_single (bytes from which a record is cut in a batch / on the per-record
    path), max_recs (the largest batch that takes a spread launch), piece (the base piece length), max_pieces."""
    out = (ctypes.c_uint32 * 4)()
    if load_library().ptls_mi355x_chacha_debug_spread_params(ctypes.cast(out, ctypes.c_void_p)) != 0:
        raise _err("ptls_mi355x_chacha_debug_spread_params")
    return {"min_batch": int(out[0]), "min_single": int(out[1]), "max_recs": int(out[2]), "piece": int(out[3]),
            "max_pieces": CHACHA_SPREAD_MAX_PIECES}


def chacha_debug_rpow(r16: bytes, e: int) -> int:
    """r^e mod 2^130 - 5 by the device's power routine, r the 16 little-endian bytes as they are
    (ptls_mi355x_chacha_debug_rpow); the fully reduced result as an integer."""
    if len(r16) != 16 or not 0 <= e < 2**64:
        raise ValueError("r is 16 bytes and e fits 64 bits")
    out = bytearray(17)
    if load_library().ptls_mi355x_chacha_debug_rpow(_buf(bytes(r16)), e, _buf(out)) != 0:
        raise _err("ptls_mi355x_chacha_debug_rpow")
    return int.from_bytes(out, "little")


def chacha_spread_plan(lens, params: dict) -> list:
    """The cuts the device plan of a spread launch makes (pure Python): for each record length the list of its pieces'
    (lo, hi) byte ranges, empty for a record that stays whole. params: "min_len" (records from this length are cut),
    "piece" (the base piece length) and "max_pieces" (the piece length doubles until a record has no more than these)."""
    plan = []
    for n in lens:
        n = int(n)
        if n < max(int(params["min_len"]), 1) or n > 1 << 30:
            plan.append([])
            continue
        piece = int(params["piece"])
        while (n + piece - 1) // piece > int(params.get("max_pieces", CHACHA_SPREAD_MAX_PIECES)):
            piece *= 2
        plan.append([(lo, min(n, lo + piece)) for lo in range(0, n, piece)])
    return plan


# ------------------------------------------------------------------------------------------------ picotls mirror


@dataclass(frozen=True)
class AeadAlgorithm:
    """Mirror of ptls_aead_algorithm_t (include/picotls.h:519-580) for ptls_mi355x_aes{128,256}gcm."""

    name: str
    key_size: int
    iv_size: int = 12
    tag_size: int = 16
    confidentiality_limit: int = 0x2000000  # PTLS_AESGCM_CONFIDENTIALITY_LIMIT, include/picotls.h:89
    integrity_limit: int = 0x40000000000000  # PTLS_AESGCM_INTEGRITY_LIMIT, include/picotls.h:90
    tls12_fixed_iv_size: int = 0
    tls12_record_iv_size: int = 0
    non_temporal: int = 0
    align_bits: int = 0


aes128gcm = AeadAlgorithm("AES128-GCM", 16)
aes256gcm = AeadAlgorithm("AES256-GCM", 32)
# ptls_mi355x_chacha20poly1305 (PTLS_CHACHA20POLY1305_* limits, include/picotls.h:98-99; TLS 1.2 IV sizes {12, 0})
chacha20poly1305 = AeadAlgorithm("CHACHA20-POLY1305", 32, confidentiality_limit=2**64 - 1, integrity_limit=2**36,
                                 tls12_fixed_iv_size=12)


class AeadContext:
    """Mirror of ptls_aead_context_t created by ptls_aead_new_direct (lib/picotls.c:6553-6568)."""

    def __init__(self, algo: AeadAlgorithm, is_enc: bool, key: bytes, iv: bytes):
        if len(key) != algo.key_size or len(iv) != algo.iv_size:
            raise ValueError("key / iv size mismatch")
        self.algo = algo
        self.is_enc = is_enc
        self._iv = bytes(iv)
        self._pfx = "ptls_mi355x_"  # the per-record calls of the algorithm's engine
        if algo.name == "CHACHA20-POLY1305":
            self._pfx = "ptls_mi355x_chacha_"
            self.ks = ChaChaKeyset(key, iv)
            return
        self.ks = Keyset(key, iv, algo.key_size)
        # as the picotls objects (ptls_mi355x.c aesgcm_setup): constant-time unless PTLS_MI355X_CONSTANT_TIME=0
        self.ks.set_constant_time(os.environ.get("PTLS_MI355X_CONSTANT_TIME") != "0")

    def free(self):
        self.ks.free()

    # do_get_iv / do_set_iv / ptls_aead_xor_iv (lib/picotls.c:6576-6585)
    def get_iv(self) -> bytes:
        return self._iv

    def set_iv(self, iv: bytes) -> None:
        self._iv = bytes(iv)
        self.ks.set_iv(self._iv)

    def xor_iv(self, data: bytes) -> None:
        iv = bytearray(self._iv)
        for i, b in enumerate(data):
            iv[i] ^= b
        self.set_iv(bytes(iv))

    # ptls_aead_encrypt (include/picotls.h:2102-2107): returns ciphertext || tag
    def encrypt(self, pt: bytes, seq: int, aad: bytes = b"") -> bytes:
        out = bytearray(len(pt) + self.algo.tag_size)
        if getattr(load_library(), self._pfx + "encrypt")(self.ks.handle, 0, _buf(out), _buf(bytes(pt)), len(pt), seq,
                                                           _buf(bytes(aad)), len(aad)) != 0:
            raise _err(self._pfx + "encrypt")
        return bytes(out)

    # ptls_aead_encrypt_v (include/picotls.h:2115-2119): the vectors sealed as one record
    def encrypt_v(self, vecs: list, seq: int, aad: bytes = b"") -> bytes:
        bufs = [bytes(v) for v in vecs]
        arr = (ctypes.c_void_p * (2 * max(len(bufs), 1)))()
        for i, b in enumerate(bufs):
            arr[2 * i] = ctypes.cast(ctypes.c_char_p(b), ctypes.c_void_p).value if b else None
            arr[2 * i + 1] = len(b)
        total = sum(len(b) for b in bufs)
        out = bytearray(total + self.algo.tag_size)
        if getattr(load_library(), self._pfx + "encrypt_v")(self.ks.handle, 0, _buf(out), ctypes.cast(arr, ctypes.c_void_p),
                                                             len(bufs), seq, _buf(bytes(aad)), len(aad)) != 0:
            raise _err(self._pfx + "encrypt_v")
        return bytes(out)

    # ptls_aead_encrypt_s with a header-protection cipher (include/picotls.h:2109-2113, lib/fusion.c:425-430,636-651):
    # the mask of the sealed sample at sample_off, computed in the seal's round trip (ptls_mi355x_encrypt_s)
    def encrypt_s(self, pt: bytes, seq: int, aad: bytes, hp: "CtrCipher", sample_off: int) -> tuple[bytes, bytes]:
        out = bytearray(len(pt) + self.algo.tag_size)
        mask = bytearray(16)
        if load_library().ptls_mi355x_encrypt_s(self.ks.handle, 0, _buf(out), _buf(bytes(pt)), len(pt), seq, _buf(bytes(aad)),
                                               len(aad), hp.ks.handle, 0, sample_off, _buf(mask)) != 0:
            raise _err("ptls_mi355x_encrypt_s")
        return bytes(out), bytes(mask)

    # ptls_aead_decrypt (include/picotls.h:2160-2164): plaintext, or None for SIZE_MAX
    def decrypt(self, ct_tag: bytes, seq: int, aad: bytes = b"", out: bytearray | None = None) -> bytes | None:
        """``out`` (optional, at least len(ct_tag) - 16 bytes): the buffer the engine writes the plaintext to."""
        if len(ct_tag) < 16:
            return None
        if out is None:
            out = bytearray(len(ct_tag) - 16 + 1)
        elif len(out) < len(ct_tag) - 16:
            raise ValueError("output buffer too small")
        r = getattr(load_library(), self._pfx + "decrypt")(self.ks.handle, 0, _buf(out), _buf(bytes(ct_tag)), len(ct_tag), seq,
                                                           _buf(bytes(aad)), len(aad))
        if r == SIZE_MAX:
            return None
        return bytes(out[:r])


class CtrCipher:
    """Mirror of ptls_mi355x_aes{128,256}ctr (fusion's 16-byte AES-CTR, lib/fusion.c:1051-1101)."""

    def __init__(self, key: bytes):
        self.ks = Keyset(key, bytes(12), len(key))

    def mask(self, iv16: bytes) -> bytes:
        out = bytearray(16)
        if load_library().ptls_mi355x_encrypt_block(self.ks.handle, 0, _buf(out), _buf(bytes(iv16))) != 0:
            raise _err("ptls_mi355x_encrypt_block")
        return bytes(out)


class ChaChaCipher:
    """Mirror of ptls_mi355x_chacha20 as QUIC header protection uses it: ptls_cipher_init with the 16-byte IV (block counter
    || nonce), then the first 16 keystream bytes."""

    def __init__(self, key: bytes):
        self.ks = ChaChaKeyset(key, bytes(12))

    def mask(self, iv16: bytes) -> bytes:
        if len(iv16) != 16:
            raise ValueError("the ChaCha20 IV is 16 bytes")
        out = bytearray(16)
        if load_library().ptls_mi355x_chacha_hp_mask(self.ks.handle, 0, _buf(out), _buf(bytes(iv16))) != 0:
            raise _err("ptls_mi355x_chacha_hp_mask")
        return bytes(out)


class QuicLbCipher:
    """Mirror of ptls_cipher_new(&ptls_mi355x_quiclb, is_enc, key) + ptls_cipher_encrypt (t/quiclb.c:36-45): the QUIC-LB
    CID cipher of lib/quiclb-impl.h, one CID of 7..19 bytes per call."""

    key_size = 16
    block_size = 8  # PTLS_QUICLB_DEFAULT_BLOCK_SIZE, include/picotls.h:119-122

    def __init__(self, is_enc: bool, key: bytes):
        if len(key) != 16:
            raise ValueError("QUIC-LB keys are 16 bytes (PTLS_QUICLB_KEY_SIZE)")
        self.is_enc = is_enc
        self.ks = Keyset(key, bytes(12), 16)

    def encrypt(self, data: bytes) -> bytes:
        if not QUICLB_MIN_LEN <= len(data) <= QUICLB_MAX_LEN:
            raise ValueError("QUIC-LB transforms 7..19 bytes")
        out = bytearray(len(data))
        if load_library().ptls_mi355x_quiclb_transform(self.ks.handle, 0, _buf(out), _buf(bytes(data)), len(data),
                                                       1 if self.is_enc else 0) != 0:
            raise _err("ptls_mi355x_quiclb_transform")
        return bytes(out)


def staging_bytes() -> int:
    """Pinned host bytes held by the per-record path's staging pools (ptls_mi355x_staging_bytes)."""
    return int(load_library().ptls_mi355x_staging_bytes())


def release_staging() -> None:
    """Frees the idle staging buffers (ptls_mi355x_release_staging)."""
    load_library().ptls_mi355x_release_staging()


# ------------------------------------------------------------------------------------------------ debug hooks


COUNTER_NAMES = ("chunked", "spread", "seal_hp", "w8_tree", "w8_serial", "lockstep", "span", "lane")


def debug_counters(reset: bool = False) -> dict:
    """ptls_mi355x_debug_counters: {"launches": {kind: n}, "runs": {kind: n}} (chunked kinds: EXT 0..4). Waits for the
    device."""
    out = (ctypes.c_uint64 * 16)()
    if load_library().ptls_mi355x_debug_counters(ctypes.cast(out, ctypes.c_void_p), 1 if reset else 0) != 0:
        raise _err("ptls_mi355x_debug_counters")
    runs = dict(zip(COUNTER_NAMES[:5], out[8:13]))
    runs["w8_g4"] = out[15]  # (of the w8_serial runs: whole runs in 4-lane groups)
    runs["w8_mk"] = out[14]  # (of the w8_serial runs: multi-key runs, round 6)
    runs["lane_records"] = out[13]  # (the records the record-per-lane kernel accepted: it has no runs)
    return {"launches": dict(zip(COUNTER_NAMES[:8], out[:8])), "runs": runs}


def debug_inject_error() -> int:
    """Leaves a HIP error as this thread's last error (ptls_mi355x_debug_inject_error); returns its code."""
    return int(load_library().ptls_mi355x_debug_inject_error())


def debug_clock_sample(dev_ptr: int, stream: int = 0) -> None:
    """Writes (s_memtime, s_memrealtime, XCC id) of the XCD the probe wave ran on (the id is out[2]) to 3 x u64 at dev_ptr,
    in stream order."""
    if load_library().ptls_mi355x_debug_clock_sample(dev_ptr, stream or None) != 0:
        raise _err("ptls_mi355x_debug_clock_sample")


def debug_wallclock_khz() -> int:
    return int(load_library().ptls_mi355x_debug_wallclock_khz())


def debug_kernel_clock(dev_ptr: int, cap: int) -> None:
    """From the next launch on, workgroup 0 of each chunked launch appends (memtime start, end, realtime start, end) as
    4 x u64 to the device buffer at dev_ptr (room for cap launches); dev_ptr 0 stops (ptls_mi355x_debug_kernel_clock)."""
    if load_library().ptls_mi355x_debug_kernel_clock(dev_ptr or None, cap if dev_ptr else 0) != 0:
        raise _err("ptls_mi355x_debug_kernel_clock")


def debug_kernel_clock_count() -> int:
    """Launches sampled since the last debug_kernel_clock (may exceed the buffer's cap)."""
    n = int(load_library().ptls_mi355x_debug_kernel_clock_count())
    if n < 0:
        raise _err("ptls_mi355x_debug_kernel_clock_count")
    return n


def aead_new_direct(algo: AeadAlgorithm, is_enc: bool, key: bytes, iv: bytes) -> AeadContext:
    return AeadContext(algo, is_enc, key, iv)


def aead_new(algo: AeadAlgorithm, hash_name: str, is_enc: bool, secret: bytes, label_prefix: str | None = None) -> AeadContext:
    """ptls_aead_new (lib/picotls.c:6529-6551): traffic key and IV from a secret (get_traffic_keys), then
    ptls_aead_new_direct. hash_name is the suite hash ("sha256", "sha384")."""
    from .keyschedule import traffic_keys

    key, iv = traffic_keys(algo.key_size, hash_name, secret, algo.iv_size, label_prefix)
    return AeadContext(algo, is_enc, key, iv)
