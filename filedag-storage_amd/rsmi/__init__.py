"""Python host mirror of filedag-storage's Dag Node erasure seam over librsmi.so.

`Erasure` mirrors dag/node/dagnode/erasure.go method for method (NewErasure,
EncodeData, DecodeDataBlocks, DecodeDataAndParityBlocks, ShardSize) with the same
argument meaning and error behaviour; every byte it produces comes out of the gfx950
HIP kernels behind the C-ABI in include/rsmi.h.  There is no CPU fallback: if the
library or a GPU is missing the calls raise.

`Codec` exposes the batched device-resident and host entry points used by bench.py.
"""
from __future__ import annotations

import ctypes
import os
from typing import List, Optional, Sequence, Tuple

_HERE = os.path.dirname(os.path.abspath(__file__))
# RSMI_LIB: a diagnostic build of the library (tools/Makefile variants) for A/B runs
LIB_PATH = os.environ.get("RSMI_LIB") or os.path.join(os.path.dirname(_HERE), "lib", "librsmi.so")

# status codes (include/rsmi.h) -- names follow the upstream sentinels
OK = 0
ErrShortData = 1
ErrTooFewShards = 2
ErrShardNoData = 3
ErrShardSize = 4
ErrInvShardNum = 5
ErrMaxShardNum = 6
ErrSingular = 7
ErrInvalidArg = 8
ErrDevice = 100
ErrNoDevice = 101
ErrHost = 102

# rsmi_locate verdicts that are not a shard index (include/rsmi.h RSMI_LOCATE_*)
LocateClean = -1
LocateUnknown = -2

# what the ragged encode does with a block (include/rsmi.h RSMI_RAGGED_*)
RaggedAligned = 0
RaggedUA = 1
RaggedFallback = 2


class RaggedBlock(ctypes.Structure):
    """include/rsmi.h rsmi_ragged_block: one block of a ragged encode."""
    _fields_ = [("S", ctypes.c_uint64), ("data_off", ctypes.c_uint64), ("data_shard_stride", ctypes.c_uint64),
                ("parity_off", ctypes.c_uint64), ("parity_shard_stride", ctypes.c_uint64)]


class RsmiError(Exception):
    def __init__(self, code: int, msg: str = ""):
        self.code = code
        super().__init__(f"rsmi error {code}: {msg or status_string(code)}")


_lib = None


def lib() -> ctypes.CDLL:
    """Load librsmi.so (fails loudly when it has not been built)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise RuntimeError(f"librsmi.so not built at {LIB_PATH}: run `python __graft_entry__.py build`")
    # One HIP runtime per process: torch ships its own libamdhip64 (soname libamdhip64.so.7).
    # Loaded first, it also satisfies librsmi's dependency; loaded after librsmi, a second
    # runtime (ROCm's) would already own the device and torch would report no GPU.
    try:
        import torch  # noqa: F401
    except ImportError:
        pass
    L = ctypes.CDLL(LIB_PATH)
    c_size = ctypes.c_size_t
    u8p = ctypes.c_void_p
    sig = {
        "rsmi_open": (ctypes.c_int, [ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.POINTER(ctypes.c_void_p)]),
        "rsmi_close": (None, [ctypes.c_void_p]),
        "rsmi_warm": (ctypes.c_int, [ctypes.c_void_p]),
        "rsmi_device_count": (ctypes.c_int, []),
        "rsmi_status_string": (ctypes.c_char_p, [ctypes.c_int]),
        "rsmi_abi_version": (ctypes.c_int, []),
        "rsmi_shard_size": (c_size, [c_size, ctypes.c_int]),
        "rsmi_recommended_pitch": (c_size, [c_size]),
        "rsmi_encode_matrix": (ctypes.c_int, [ctypes.c_void_p, u8p]),
        "rsmi_check_shards": (ctypes.c_int, [ctypes.c_int, ctypes.POINTER(c_size), ctypes.c_int, ctypes.POINTER(c_size)]),
        "rsmi_decode_matrix": (ctypes.c_int, [ctypes.c_void_p, u8p, u8p, ctypes.POINTER(ctypes.c_int)]),
        "rsmi_encode_block": (ctypes.c_int, [ctypes.c_void_p, u8p, c_size, u8p]),
        "rsmi_encode": (ctypes.c_int, [ctypes.c_void_p, u8p, u8p, c_size]),
        "rsmi_reconstruct": (ctypes.c_int, [ctypes.c_void_p, u8p, c_size, u8p, ctypes.c_int]),
        "rsmi_encode_batch_host": (ctypes.c_int, [ctypes.c_void_p, u8p, c_size, u8p, c_size, c_size, c_size]),
        "rsmi_reconstruct_batch_host": (ctypes.c_int, [ctypes.c_void_p, u8p, c_size, c_size, c_size, u8p, ctypes.c_int]),
        "rsmi_reconstruct_rows_batch_host": (ctypes.c_int, [ctypes.c_void_p, u8p, c_size, c_size, c_size, u8p, u8p]),
        "rsmi_reconstruct_rows_batch_dev": (ctypes.c_int, [ctypes.c_void_p, u8p, c_size, c_size, c_size, c_size, u8p, u8p, ctypes.c_void_p]),
        "rsmi_host_alloc": (ctypes.c_void_p, [c_size]),
        "rsmi_host_free": (None, [ctypes.c_void_p]),
        "rsmi_encode_batch_dev": (ctypes.c_int, [ctypes.c_void_p, u8p, c_size, c_size, u8p, c_size, c_size, c_size, c_size, ctypes.c_void_p]),
        "rsmi_reconstruct_batch_dev": (ctypes.c_int, [ctypes.c_void_p, u8p, c_size, c_size, c_size, c_size, u8p, ctypes.c_int, ctypes.c_void_p]),
        "rsmi_reconstruct_mixed_batch_dev": (ctypes.c_int, [ctypes.c_void_p, u8p, c_size, c_size, c_size, c_size, u8p, u8p,
                                                            ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p]),
        "rsmi_reconstruct_mixed_batch_host": (ctypes.c_int, [ctypes.c_void_p, u8p, c_size, c_size, c_size, u8p, u8p,
                                                             ctypes.c_int, ctypes.c_void_p]),
        "rsmi_reconstruct_mixed_batch_dev_crcs": (ctypes.c_int, [ctypes.c_void_p, u8p, c_size, c_size, c_size, c_size, u8p,
                                                                 u8p, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p,
                                                                 ctypes.c_void_p, ctypes.c_void_p]),
        "rsmi_reconstruct_mixed_batch_host_crcs": (ctypes.c_int, [ctypes.c_void_p, u8p, c_size, c_size, c_size, u8p, u8p,
                                                                  ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p,
                                                                  ctypes.c_void_p]),
        "rsmi_reconstruct_mixed_batch_dev_verify": (ctypes.c_int, [ctypes.c_void_p, u8p, c_size, c_size, c_size, c_size, u8p,
                                                                   u8p, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p,
                                                                   ctypes.c_void_p]),
        "rsmi_reconstruct_mixed_batch_host_verify": (ctypes.c_int, [ctypes.c_void_p, u8p, c_size, c_size, c_size, u8p, u8p,
                                                                    ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p]),
        "rsmi_crc_named_rows_dev": (ctypes.c_int, [ctypes.c_void_p, u8p, c_size, c_size, u8p, c_size, c_size, c_size, c_size,
                                                   ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p,
                                                   ctypes.c_void_p]),
        "rsmi_reconstruct_mixed_classify": (ctypes.c_int, [ctypes.c_void_p, c_size, u8p, u8p, ctypes.c_int,
                                                           ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
                                                           ctypes.POINTER(c_size)]),
        "rsmi_encode_ragged_batch_dev": (ctypes.c_int, [ctypes.c_void_p, u8p, u8p, ctypes.c_void_p, c_size,
                                                        ctypes.c_void_p]),
        "rsmi_encode_ragged_batch_host": (ctypes.c_int, [ctypes.c_void_p, u8p, u8p, ctypes.c_void_p, c_size]),
        "rsmi_encode_ragged_classify": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
                                                       ctypes.c_void_p, c_size, ctypes.c_void_p, ctypes.c_void_p]),
        "rsmi_verify_batch_dev": (ctypes.c_int, [ctypes.c_void_p, u8p, c_size, c_size, u8p, c_size, c_size, c_size, c_size,
                                                 ctypes.c_void_p, ctypes.c_void_p]),
        "rsmi_verify_batch_host": (ctypes.c_int, [ctypes.c_void_p, u8p, c_size, u8p, c_size, c_size, c_size,
                                                  ctypes.c_void_p]),
        "rsmi_verify": (ctypes.c_int, [ctypes.c_void_p, u8p, c_size, ctypes.POINTER(ctypes.c_int)]),
        "rsmi_scrub_batch_dev": (ctypes.c_int, [ctypes.c_void_p, u8p, c_size, c_size, u8p, c_size, c_size, c_size, c_size,
                                                ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]),
        "rsmi_scrub_batch_host": (ctypes.c_int, [ctypes.c_void_p, u8p, c_size, u8p, c_size, c_size, c_size,
                                                 ctypes.c_void_p, ctypes.c_void_p]),
        "rsmi_scrub": (ctypes.c_int, [ctypes.c_void_p, u8p, c_size, ctypes.POINTER(ctypes.c_int), ctypes.c_void_p]),
        "rsmi_locate_batch_dev": (ctypes.c_int, [ctypes.c_void_p, u8p, c_size, c_size, u8p, c_size, c_size, c_size, c_size,
                                                 ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]),
        "rsmi_locate_batch_host": (ctypes.c_int, [ctypes.c_void_p, u8p, c_size, u8p, c_size, c_size, c_size,
                                                  ctypes.c_void_p, ctypes.c_void_p]),
        "rsmi_locate": (ctypes.c_int, [ctypes.c_void_p, u8p, c_size, ctypes.POINTER(ctypes.c_int)]),
        "rsmi_locate_matrix": (ctypes.c_int, [ctypes.c_void_p, u8p]),
        "rsmi_locate_pair_batch_dev": (ctypes.c_int, [ctypes.c_void_p, u8p, c_size, c_size, u8p, c_size, c_size, c_size,
                                                      c_size, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]),
        "rsmi_locate_pair_batch_host": (ctypes.c_int, [ctypes.c_void_p, u8p, c_size, u8p, c_size, c_size, c_size,
                                                       ctypes.c_void_p, ctypes.c_void_p]),
        "rsmi_locate_pair": (ctypes.c_int, [ctypes.c_void_p, u8p, c_size, ctypes.POINTER(ctypes.c_int)]),
        "rsmi_locate_pair_checks": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int, ctypes.c_int, u8p]),
        "rsmi_heal_batch_dev": (ctypes.c_int, [ctypes.c_void_p, u8p, c_size, c_size, u8p, c_size, c_size, c_size, c_size,
                                               ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]),
        "rsmi_heal_batch_host": (ctypes.c_int, [ctypes.c_void_p, u8p, c_size, u8p, c_size, c_size, c_size,
                                                ctypes.c_void_p, ctypes.c_void_p]),
        "rsmi_heal": (ctypes.c_int, [ctypes.c_void_p, u8p, c_size, ctypes.POINTER(ctypes.c_int)]),
        "rsmi_heal_pair_batch_dev": (ctypes.c_int, [ctypes.c_void_p, u8p, c_size, c_size, u8p, c_size, c_size, c_size,
                                                    c_size, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]),
        "rsmi_heal_pair_batch_host": (ctypes.c_int, [ctypes.c_void_p, u8p, c_size, u8p, c_size, c_size, c_size,
                                                     ctypes.c_void_p, ctypes.c_void_p]),
        "rsmi_heal_pair": (ctypes.c_int, [ctypes.c_void_p, u8p, c_size, ctypes.POINTER(ctypes.c_int)]),
        "rsmi_heal_pair_matrix": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int, ctypes.c_int, u8p]),
        "rsmi_encode_block_coalesced": (ctypes.c_int, [ctypes.c_void_p, u8p, c_size, u8p, ctypes.c_void_p]),
        "rsmi_encode_block_coalesced_crcs": (ctypes.c_int, [ctypes.c_void_p, u8p, c_size, u8p, ctypes.c_void_p,
                                                            ctypes.c_void_p]),
        "rsmi_reconstruct_coalesced": (ctypes.c_int, [ctypes.c_void_p, u8p, c_size, u8p, ctypes.c_int]),
        "rsmi_get_stat": (ctypes.c_long, [ctypes.c_void_p, ctypes.c_char_p]),
        "rsmi_crc16_ibm": (ctypes.c_uint16, [u8p, c_size]),
        "rsmi_crc16_entry": (ctypes.c_uint16, [u8p, c_size, ctypes.c_uint32, c_size]),
        "rsmi_crc16_rows_dev": (ctypes.c_int, [ctypes.c_void_p, u8p, c_size, c_size, ctypes.c_int, c_size, c_size,
                                               ctypes.c_void_p, c_size, ctypes.c_void_p]),
        "rsmi_encode_batch_host_crc": (ctypes.c_int, [ctypes.c_void_p, u8p, c_size, u8p, c_size, c_size, c_size,
                                                      ctypes.c_void_p]),
        "rsmi_encode_block_crc": (ctypes.c_int, [ctypes.c_void_p, u8p, c_size, u8p, ctypes.c_void_p]),
        "rsmi_encode_batch_dev_crc": (ctypes.c_int, [ctypes.c_void_p, u8p, c_size, c_size, u8p, c_size, c_size, c_size,
                                                     c_size, ctypes.c_void_p, ctypes.c_void_p]),
        "rsmi_crc_rows_host": (ctypes.c_int, [ctypes.c_void_p, u8p, c_size, c_size, c_size, ctypes.c_void_p,
                                              ctypes.c_void_p]),
        "rsmi_crc32_ieee": (ctypes.c_uint32, [u8p, c_size]),
        "rsmi_crc32_entry": (ctypes.c_uint32, [u8p, c_size, ctypes.c_uint32, c_size]),
        "rsmi_crc32_rows_dev": (ctypes.c_int, [ctypes.c_void_p, u8p, c_size, c_size, ctypes.c_int, c_size, c_size,
                                               ctypes.c_void_p, c_size, ctypes.c_void_p]),
        "rsmi_encode_batch_host_crcs": (ctypes.c_int, [ctypes.c_void_p, u8p, c_size, u8p, c_size, c_size, c_size,
                                                       ctypes.c_void_p, ctypes.c_void_p]),
        "rsmi_reconstruct_batch_host_verify": (ctypes.c_int, [ctypes.c_void_p, u8p, c_size, c_size, c_size, u8p,
                                                              ctypes.c_int, ctypes.c_void_p]),
        "rsmi_reconstruct_rows_batch_host_crcs": (ctypes.c_int, [ctypes.c_void_p, u8p, c_size, c_size, c_size, u8p,
                                                                 u8p, ctypes.c_void_p, ctypes.c_void_p]),
        "rsmi_set_option": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_char_p, ctypes.c_long]),
        "rsmi_group_open": (ctypes.c_int, [ctypes.c_int, ctypes.c_int, ctypes.POINTER(ctypes.c_int), ctypes.c_int,
                                         ctypes.POINTER(ctypes.c_void_p)]),
        "rsmi_group_close": (None, [ctypes.c_void_p]),
        "rsmi_group_size": (ctypes.c_int, [ctypes.c_void_p]),
        "rsmi_group_context": (ctypes.c_void_p, [ctypes.c_void_p, ctypes.c_int]),
        "rsmi_partition": (ctypes.c_int, [c_size, ctypes.c_int, ctypes.c_int, ctypes.POINTER(c_size),
                                          ctypes.POINTER(c_size)]),
        "rsmi_key_slot": (ctypes.c_int, [u8p, c_size]),
        "rsmi_group_member_of_key": (ctypes.c_int, [ctypes.c_void_p, u8p, c_size]),
        "rsmi_group_member_numa_node": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int]),
        "rsmi_group_host_alloc": (ctypes.c_void_p, [ctypes.c_void_p, c_size, c_size]),
        "rsmi_group_host_free": (None, [ctypes.c_void_p, ctypes.c_void_p]),
        "rsmi_device_numa_node": (ctypes.c_int, [ctypes.c_int]),
        "rsmi_sysfs_numa_node": (ctypes.c_int, [ctypes.c_char_p, ctypes.c_char_p]),
        "rsmi_sysfs_node_cpus": (ctypes.c_int, [ctypes.c_char_p, ctypes.c_int, ctypes.POINTER(ctypes.c_int),
                                                ctypes.c_int]),
        "rsmi_bind_thread_to_numa_node": (ctypes.c_int, [ctypes.c_int]),
        "rsmi_group_encode_batch_host": (ctypes.c_int, [ctypes.c_void_p, u8p, c_size, u8p, c_size, c_size, c_size]),
        "rsmi_group_encode_batch_host_crcs": (ctypes.c_int, [ctypes.c_void_p, u8p, c_size, u8p, c_size, c_size, c_size,
                                                           ctypes.c_void_p, ctypes.c_void_p]),
        "rsmi_group_reconstruct_batch_host": (ctypes.c_int, [ctypes.c_void_p, u8p, c_size, c_size, c_size, u8p,
                                                           ctypes.c_int]),
        "rsmi_group_reconstruct_rows_batch_host": (ctypes.c_int, [ctypes.c_void_p, u8p, c_size, c_size, c_size, u8p,
                                                                u8p]),
        "rsmi_last_kernel": (ctypes.c_char_p, [ctypes.c_void_p]),
        "rsmi_set_wait_hook": (None, [ctypes.c_void_p, ctypes.c_void_p]),
        "rsmi_run_wait_hook": (ctypes.c_int, []),
    }
    for name, (res, args) in sig.items():
        f = getattr(L, name)
        f.restype = res
        f.argtypes = args
    _lib = L
    return L


def status_string(code: int) -> str:
    try:
        return lib().rsmi_status_string(code).decode()
    except Exception:  # pragma: no cover - only when the library is absent
        return "unknown"


def _check(rc: int) -> None:
    if rc != OK:
        raise RsmiError(rc)


def ceil_frac(numerator: int, denominator: int) -> int:
    """utils.go:6-21 ceilFrac."""
    if denominator == 0:
        return 0
    if denominator < 0:
        numerator, denominator = -numerator, -denominator
    q = abs(numerator) // denominator * (1 if numerator >= 0 else -1)
    if numerator > 0 and numerator % denominator != 0:
        q += 1
    return q


def _buf(b) -> ctypes.Array:
    return (ctypes.c_uint8 * len(b)).from_buffer(b)


class Codec:
    """One RS(k, m) context on one device (rsmi_open)."""

    def __init__(self, k: int, m: int, device: int = 0):
        h = ctypes.c_void_p()
        _check(lib().rsmi_open(k, m, device, ctypes.byref(h)))
        self.k, self.m, self.n, self.device = k, m, k + m, device
        self._h = h

    def close(self) -> None:
        if self._h:
            lib().rsmi_close(self._h)
            self._h = ctypes.c_void_p()

    def __del__(self):  # pragma: no cover
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    # -- host-only helpers
    def encode_matrix(self) -> bytes:
        out = bytearray(self.n * self.k)
        _check(lib().rsmi_encode_matrix(self._h, ctypes.addressof(_buf(out))))
        return bytes(out)

    def decode_matrix(self, present: Sequence[bool]):
        p = bytearray(1 if x else 0 for x in present)
        out = bytearray(self.k * self.k)
        used = (ctypes.c_int * self.k)()
        _check(lib().rsmi_decode_matrix(self._h, ctypes.addressof(_buf(p)), ctypes.addressof(_buf(out)), used))
        return bytes(out), list(used)

    def locate_matrix(self) -> bytes:
        """rsmi_locate_matrix: the m x k ratio matrix R[j][c] = M[k+j][c] / M[k][c], row-major."""
        out = bytearray(self.m * self.k)
        _check(lib().rsmi_locate_matrix(self._h, ctypes.addressof(_buf(out))))
        return bytes(out)

    def locate_pair_checks(self, x: int, y: int) -> bytes:
        """rsmi_locate_pair_checks: (m - 2) x m check rows C, row-major, with C h_x = C h_y = 0 for the
        columns of H = [M | I]; the pair {x, y} explains a byte column iff C syn = 0.  Empty for m <= 2."""
        out = bytearray(max(0, self.m - 2) * self.m)
        scratch = out if out else bytearray(1)  # the call needs a pointer and writes nothing for m <= 2
        _check(lib().rsmi_locate_pair_checks(self._h, x, y, ctypes.addressof(_buf(scratch))))
        return bytes(out)

    def heal_pair_matrix(self, x: int, y: int) -> bytes:
        """rsmi_heal_pair_matrix: the 2 x m matrix D, row-major, with D h_x = (1, 0) and D h_y = (0, 1) for
        the columns of H = [M | I]; D syn is (row x's error, row y's error) where {x, y} explains."""
        out = bytearray(2 * self.m)
        _check(lib().rsmi_heal_pair_matrix(self._h, x, y, ctypes.addressof(_buf(out))))
        return bytes(out)

    def set_option(self, key: str, value: int) -> None:
        """rsmi_set_option (include/rsmi.h lists every key).  Among them: waves_per_cu (grid cap),
        small_call_bytes, zero_copy, the folds crc16_fold / crc16_fused_fold / crc32_fold, the
        coalesce_* keys, and launch_units_max: the most tiles (or, for the fused encode + CRC-16
        and scrub, units of 4 tiles) one kernel launch takes, 1 to 2^24 - 1 (the default; 0 restores
        it); a longer batch runs as several launches of whole blocks.  stat("launch_units_max")
        reports the value in force and stat("split_launches") counts those launches.  An unknown key
        or a value out of range raises RsmiError(ErrInvalidArg)."""
        _check(lib().rsmi_set_option(self._h, key.encode(), int(value)))

    def warm(self) -> None:
        """rsmi_warm: bind the device and bring up every coalescing lane now."""
        _check(lib().rsmi_warm(self._h))

    def last_kernel(self) -> str:
        return lib().rsmi_last_kernel(self._h).decode()

    # -- host memory
    def encode_block(self, block: bytes) -> bytes:
        S = lib().rsmi_shard_size(len(block), self.k)
        out = bytearray(self.n * S)
        src = bytearray(block)
        _check(lib().rsmi_encode_block(self._h, ctypes.addressof(_buf(src)) if src else None, len(block),
                                       ctypes.addressof(_buf(out)) if out else None))
        return bytes(out)

    def encode(self, data: bytearray, parity: bytearray, S: int) -> None:
        _check(lib().rsmi_encode(self._h, ctypes.addressof(_buf(data)), ctypes.addressof(_buf(parity)), S))

    def reconstruct(self, shards: bytearray, S: int, present: Sequence[bool], data_only: bool) -> None:
        p = bytearray(1 if x else 0 for x in present)
        _check(lib().rsmi_reconstruct(self._h, ctypes.addressof(_buf(shards)), S, ctypes.addressof(_buf(p)),
                                      1 if data_only else 0))

    def encode_batch_host_ptr(self, data_ptr: int, data_bs: int, parity_ptr: int, parity_bs: int, S: int,
                              nblocks: int) -> None:
        _check(lib().rsmi_encode_batch_host(self._h, data_ptr, data_bs, parity_ptr, parity_bs, S, nblocks))

    def verify(self, shards, S: int) -> bool:
        """Encoder.Verify of one block of n*S contiguous bytes: True iff every parity row is the
        encode of the data rows (rsmi_verify)."""
        src = shards if isinstance(shards, bytearray) else bytearray(shards)
        ok = ctypes.c_int(-1)
        _check(lib().rsmi_verify(self._h, ctypes.addressof(_buf(src)) if src else None, S, ctypes.byref(ok)))
        return ok.value == 1

    def verify_batch_host_ptr(self, data_ptr: int, data_bs: int, parity_ptr: int, parity_bs: int, S: int,
                              nblocks: int, bad_ptr: int) -> None:
        """rsmi_verify_batch_host: bad_ptr[b*m + j] (uint32, host memory) non-zero iff parity row j
        of block b differs from the encode of the block's data rows."""
        _check(lib().rsmi_verify_batch_host(self._h, data_ptr, data_bs, parity_ptr, parity_bs, S, nblocks, bad_ptr))

    def scrub(self, shards, S: int) -> Tuple[bool, List[int]]:
        """rsmi_scrub of one block of n*S contiguous bytes: (verify's answer, R(shard) of each of
        the n shards as stored), from one read of the rows."""
        src = shards if isinstance(shards, bytearray) else bytearray(shards)
        ok = ctypes.c_int(-1)
        raw = (ctypes.c_uint32 * self.n)()
        _check(lib().rsmi_scrub(self._h, ctypes.addressof(_buf(src)) if src else None, S, ctypes.byref(ok), raw))
        return ok.value == 1, list(raw)

    def scrub_batch_host_ptr(self, data_ptr: int, data_bs: int, parity_ptr: int, parity_bs: int, S: int,
                             nblocks: int, bad_ptr: int, raw_ptr: int) -> None:
        """rsmi_scrub_batch_host: rsmi_verify_batch_host's flags in bad_ptr[b*m + j] and R(row) in
        raw_ptr[b*n + r] (uint32, host memory, data rows first)."""
        _check(lib().rsmi_scrub_batch_host(self._h, data_ptr, data_bs, parity_ptr, parity_bs, S, nblocks,
                                           bad_ptr or None, raw_ptr or None))

    def locate(self, shards, S: int) -> int:
        """rsmi_locate of one block of n*S contiguous bytes: LocateClean, the index of the one
        shard that explains the damage, or LocateUnknown."""
        src = shards if isinstance(shards, bytearray) else bytearray(shards)
        v = ctypes.c_int(LocateUnknown)
        _check(lib().rsmi_locate(self._h, ctypes.addressof(_buf(src)) if src else None, S, ctypes.byref(v)))
        return v.value

    def locate_batch_host_ptr(self, data_ptr: int, data_bs: int, parity_ptr: int, parity_bs: int, S: int,
                              nblocks: int, culprit_ptr: int, bad_ptr: int = 0) -> None:
        """rsmi_locate_batch_host: culprit_ptr[b] (int32, host memory) and, when bad_ptr is given,
        rsmi_verify_batch_host's flags."""
        _check(lib().rsmi_locate_batch_host(self._h, data_ptr, data_bs, parity_ptr, parity_bs, S, nblocks,
                                            culprit_ptr, bad_ptr or None))

    def locate_pair(self, shards, S: int) -> Tuple[int, int]:
        """rsmi_locate_pair of one block of n*S contiguous bytes: (-1, -1) clean, (x, -1) the single
        shard rsmi_locate names, (x, y) the one pair of shards that explains the damage, or (-2, -2)."""
        src = shards if isinstance(shards, bytearray) else bytearray(shards)
        v = (ctypes.c_int * 2)(LocateUnknown, LocateUnknown)
        _check(lib().rsmi_locate_pair(self._h, ctypes.addressof(_buf(src)) if src else None, S, v))
        return v[0], v[1]

    def locate_pair_batch_host_ptr(self, data_ptr: int, data_bs: int, parity_ptr: int, parity_bs: int, S: int,
                                   nblocks: int, pair_ptr: int, bad_ptr: int = 0) -> None:
        """rsmi_locate_pair_batch_host: pair_ptr[2b], pair_ptr[2b+1] (int32, host memory) and, when
        bad_ptr is given, rsmi_verify_batch_host's flags."""
        _check(lib().rsmi_locate_pair_batch_host(self._h, data_ptr, data_bs, parity_ptr, parity_bs, S, nblocks,
                                                 pair_ptr, bad_ptr or None))

    def heal(self, shards: bytearray, S: int) -> int:
        """rsmi_heal of one block of n*S contiguous bytes, healed in place: the verdict of the
        block as it was (rsmi_locate's); when it names a shard, that row of shards is rewritten
        so that the stripe is clean, and nothing else is."""
        if not isinstance(shards, bytearray):
            raise TypeError("heal rewrites its argument: pass a bytearray")
        v = ctypes.c_int(LocateUnknown)
        _check(lib().rsmi_heal(self._h, ctypes.addressof(_buf(shards)) if shards else None, S, ctypes.byref(v)))
        return v.value

    def heal_batch_host_ptr(self, data_ptr: int, data_bs: int, parity_ptr: int, parity_bs: int, S: int,
                            nblocks: int, culprit_ptr: int, bad_ptr: int = 0) -> None:
        """rsmi_heal_batch_host: rsmi_locate_batch_host's outputs, and the named row of every block
        that has one rewritten in the caller's buffers."""
        _check(lib().rsmi_heal_batch_host(self._h, data_ptr, data_bs, parity_ptr, parity_bs, S, nblocks,
                                          culprit_ptr, bad_ptr or None))

    def heal_pair(self, shards: bytearray, S: int) -> Tuple[int, int]:
        """rsmi_heal_pair of one block of n*S contiguous bytes, healed in place: the verdict of the
        block as it was (rsmi_locate_pair's); the one or two rows it names are rewritten so that
        the stripe is clean, and nothing else is."""
        if not isinstance(shards, bytearray):
            raise TypeError("heal_pair rewrites its argument: pass a bytearray")
        v = (ctypes.c_int * 2)(LocateUnknown, LocateUnknown)
        _check(lib().rsmi_heal_pair(self._h, ctypes.addressof(_buf(shards)) if shards else None, S, v))
        return v[0], v[1]

    def heal_pair_batch_host_ptr(self, data_ptr: int, data_bs: int, parity_ptr: int, parity_bs: int, S: int,
                                 nblocks: int, pair_ptr: int, bad_ptr: int = 0) -> None:
        """rsmi_heal_pair_batch_host: rsmi_locate_pair_batch_host's outputs, and the one or two named
        rows of every block that has any rewritten in the caller's buffers."""
        _check(lib().rsmi_heal_pair_batch_host(self._h, data_ptr, data_bs, parity_ptr, parity_bs, S, nblocks,
                                               pair_ptr, bad_ptr or None))

    def reconstruct_batch_host_ptr(self, ptr: int, bs: int, S: int, nblocks: int, present: Sequence[bool],
                                   data_only: bool) -> None:
        p = bytearray(1 if x else 0 for x in present)
        _check(lib().rsmi_reconstruct_batch_host(self._h, ptr, bs, S, nblocks, ctypes.addressof(_buf(p)),
                                                 1 if data_only else 0))

    def reconstruct_rows_batch_host_ptr(self, ptr: int, bs: int, S: int, nblocks: int, present: Sequence[bool],
                                        required: Sequence[bool]) -> None:
        p = bytearray(1 if x else 0 for x in present)
        q = bytearray(1 if x else 0 for x in required)
        _check(lib().rsmi_reconstruct_rows_batch_host(self._h, ptr, bs, S, nblocks, ctypes.addressof(_buf(p)),
                                                      ctypes.addressof(_buf(q))))

    def encode_block_crc(self, block: bytes):
        """encode_block plus R(shard) of every shard (GPU CRC-16, include/rsmi.h)."""
        S = lib().rsmi_shard_size(len(block), self.k)
        out = bytearray(self.n * S)
        src = bytearray(block)
        raw = (ctypes.c_uint32 * self.n)()
        _check(lib().rsmi_encode_block_crc(self._h, ctypes.addressof(_buf(src)) if src else None, len(block),
                                           ctypes.addressof(_buf(out)) if out else None, raw))
        return bytes(out), list(raw)

    def encode_block_coalesced(self, block: bytes, want_raw: bool = False):
        """encode_block, batched with concurrent callers on this context (group commit)."""
        S = lib().rsmi_shard_size(len(block), self.k)
        out = bytearray(self.n * S)
        src = bytearray(block)
        raw = (ctypes.c_uint32 * self.n)() if want_raw else None
        _check(lib().rsmi_encode_block_coalesced(self._h, ctypes.addressof(_buf(src)) if src else None, len(block),
                                                 ctypes.addressof(_buf(out)) if out else None, raw))
        return (bytes(out), list(raw)) if want_raw else bytes(out)

    def reconstruct_coalesced(self, shards: bytearray, S: int, present: Sequence[bool], data_only: bool) -> None:
        """reconstruct, batched with concurrent callers on this context (group commit)."""
        p = bytearray(1 if x else 0 for x in present)
        _check(lib().rsmi_reconstruct_coalesced(self._h, ctypes.addressof(_buf(shards)), S,
                                                ctypes.addressof(_buf(p)), 1 if data_only else 0))

    def stat(self, key: str) -> int:
        """rsmi_get_stat: the coalesced_* counters, launch_units_max, split_launches; -1 for an
        unknown key."""
        return lib().rsmi_get_stat(self._h, key.encode())

    def encode_batch_host_crc_ptr(self, data_ptr: int, data_bs: int, parity_ptr: int, parity_bs: int, S: int,
                                  nblocks: int, raw_ptr: int) -> None:
        _check(lib().rsmi_encode_batch_host_crc(self._h, data_ptr, data_bs, parity_ptr, parity_bs, S, nblocks,
                                                raw_ptr))

    def encode_batch_dev_crc(self, d_data: int, data_rs: int, data_bs: int, d_parity: int, parity_rs: int,
                             parity_bs: int, S: int, nblocks: int, d_raw: int, stream: int = 0) -> None:
        _check(lib().rsmi_encode_batch_dev_crc(self._h, d_data, data_rs, data_bs, d_parity, parity_rs, parity_bs, S,
                                               nblocks, d_raw, stream or None))

    def crc16_rows_dev(self, d_rows: int, rs: int, bs: int, nrows: int, S: int, nblocks: int, d_out: int,
                       out_bs: int, stream: int = 0) -> None:
        _check(lib().rsmi_crc16_rows_dev(self._h, d_rows, rs, bs, nrows, S, nblocks, d_out, out_bs,
                                         stream or None))

    def crc_rows_host_ptr(self, rows_ptr: int, row_stride: int, nrows: int, S: int, raw16_ptr: Optional[int],
                          raw32_ptr: Optional[int]) -> None:
        _check(lib().rsmi_crc_rows_host(self._h, rows_ptr, row_stride, nrows, S, raw16_ptr or None,
                                        raw32_ptr or None))

    def crc32_rows_dev(self, d_rows: int, rs: int, bs: int, nrows: int, S: int, nblocks: int, d_out: int,
                       out_bs: int, stream: int = 0) -> None:
        """R32(row) of the mutcask value checksum (CRC-32 IEEE, raw) for every row, on the device."""
        _check(lib().rsmi_crc32_rows_dev(self._h, d_rows, rs, bs, nrows, S, nblocks, d_out, out_bs,
                                         stream or None))

    def reconstruct_batch_host_verify_ptr(self, ptr: int, bs: int, S: int, nblocks: int, present: Sequence[bool],
                                          data_only: bool, raw16_ptr: int) -> None:
        """reconstruct_batch_host_ptr that also writes R(row) of the k survivor rows it read into
        raw16_ptr[b*k + c] (uint32; survivors = the first k present shards)."""
        p = bytearray(1 if x else 0 for x in present)
        _check(lib().rsmi_reconstruct_batch_host_verify(self._h, ptr, bs, S, nblocks, ctypes.addressof(_buf(p)),
                                                        1 if data_only else 0, raw16_ptr))

    def reconstruct_rows_batch_host_crcs_ptr(self, shards_ptr: int, block_stride: int, S: int, nblocks: int,
                                             present: Sequence[bool], required: Sequence[bool],
                                             raw16_ptr: Optional[int], raw32_ptr: Optional[int]) -> None:
        p = bytearray(1 if x else 0 for x in present)
        q = bytearray(1 if x else 0 for x in required)
        _check(lib().rsmi_reconstruct_rows_batch_host_crcs(self._h, shards_ptr, block_stride, S, nblocks,
                                                           ctypes.addressof(_buf(p)), ctypes.addressof(_buf(q)),
                                                           raw16_ptr or None, raw32_ptr or None))

    def encode_batch_host_crcs_ptr(self, data_ptr: int, data_bs: int, parity_ptr: int, parity_bs: int, S: int,
                                   nblocks: int, raw16_ptr: Optional[int], raw32_ptr: Optional[int]) -> None:
        _check(lib().rsmi_encode_batch_host_crcs(self._h, data_ptr, data_bs, parity_ptr, parity_bs, S, nblocks,
                                                 raw16_ptr or None, raw32_ptr or None))

    # -- device memory (raw pointers, e.g. torch tensor.data_ptr()); stream = hipStream_t
    def encode_batch_dev(self, d_data: int, data_rs: int, data_bs: int, d_parity: int, parity_rs: int,
                         parity_bs: int, S: int, nblocks: int, stream: int = 0) -> None:
        _check(lib().rsmi_encode_batch_dev(self._h, d_data, data_rs, data_bs, d_parity, parity_rs, parity_bs, S,
                                           nblocks, stream or None))

    def verify_batch_dev(self, d_data: int, data_rs: int, data_bs: int, d_parity: int, parity_rs: int,
                         parity_bs: int, S: int, nblocks: int, d_bad: int, stream: int = 0) -> None:
        """rsmi_verify_batch_dev: d_bad[b*m + j] (uint32, device memory, zeroed on the stream first)
        non-zero iff stored parity row j of block b is not the encode of the block's data rows."""
        _check(lib().rsmi_verify_batch_dev(self._h, d_data, data_rs, data_bs, d_parity, parity_rs, parity_bs, S,
                                           nblocks, d_bad, stream or None))

    def scrub_batch_dev(self, d_data: int, data_rs: int, data_bs: int, d_parity: int, parity_rs: int,
                        parity_bs: int, S: int, nblocks: int, d_bad: int, d_raw: int, stream: int = 0) -> None:
        """rsmi_scrub_batch_dev: rsmi_verify_batch_dev's flags in d_bad[b*m + j] and what
        rsmi_crc16_rows_dev writes for every row in d_raw[b*n + r] (uint32, device memory, data rows
        first), from one read of the rows.  Stream-ordered."""
        _check(lib().rsmi_scrub_batch_dev(self._h, d_data, data_rs, data_bs, d_parity, parity_rs, parity_bs, S,
                                          nblocks, d_bad or None, d_raw or None, stream or None))

    def locate_batch_dev(self, d_data: int, data_rs: int, data_bs: int, d_parity: int, parity_rs: int,
                         parity_bs: int, S: int, nblocks: int, d_culprit: int, d_bad: int = 0, stream: int = 0) -> None:
        """rsmi_locate_batch_dev: d_culprit[b] (int32, device memory) and, when d_bad is given,
        rsmi_verify_batch_dev's flags, from one pass over the rows."""
        _check(lib().rsmi_locate_batch_dev(self._h, d_data, data_rs, data_bs, d_parity, parity_rs, parity_bs, S,
                                           nblocks, d_culprit, d_bad or None, stream or None))

    def locate_pair_batch_dev(self, d_data: int, data_rs: int, data_bs: int, d_parity: int, parity_rs: int,
                              parity_bs: int, S: int, nblocks: int, d_pair: int, d_bad: int = 0,
                              stream: int = 0) -> None:
        """rsmi_locate_pair_batch_dev: d_pair[2b], d_pair[2b+1] (int32, device memory) and, when d_bad
        is given, rsmi_verify_batch_dev's flags.  Stream-ordered."""
        _check(lib().rsmi_locate_pair_batch_dev(self._h, d_data, data_rs, data_bs, d_parity, parity_rs, parity_bs, S,
                                                nblocks, d_pair, d_bad or None, stream or None))

    def heal_batch_dev(self, d_data: int, data_rs: int, data_bs: int, d_parity: int, parity_rs: int,
                       parity_bs: int, S: int, nblocks: int, d_culprit: int, d_bad: int = 0, stream: int = 0) -> None:
        """rsmi_heal_batch_dev: rsmi_locate_batch_dev's outputs, then, behind them on the stream,
        the named row of every block that has one rewritten so that the stripe is clean."""
        _check(lib().rsmi_heal_batch_dev(self._h, d_data, data_rs, data_bs, d_parity, parity_rs, parity_bs, S,
                                         nblocks, d_culprit, d_bad or None, stream or None))

    def heal_pair_batch_dev(self, d_data: int, data_rs: int, data_bs: int, d_parity: int, parity_rs: int,
                            parity_bs: int, S: int, nblocks: int, d_pair: int, d_bad: int = 0, stream: int = 0) -> None:
        """rsmi_heal_pair_batch_dev: rsmi_locate_pair_batch_dev's outputs, then, behind them on the
        stream, the one or two named rows of every block that has any rewritten so that the stripe is
        clean."""
        _check(lib().rsmi_heal_pair_batch_dev(self._h, d_data, data_rs, data_bs, d_parity, parity_rs, parity_bs, S,
                                              nblocks, d_pair, d_bad or None, stream or None))

    def reconstruct_rows_batch_dev(self, d_shards: int, rs: int, bs: int, S: int, nblocks: int,
                                   present: Sequence[bool], required: Sequence[bool], stream: int = 0) -> None:
        p = bytearray(1 if x else 0 for x in present)
        q = bytearray(1 if x else 0 for x in required)
        _check(lib().rsmi_reconstruct_rows_batch_dev(self._h, d_shards, rs, bs, S, nblocks, ctypes.addressof(_buf(p)),
                                                     ctypes.addressof(_buf(q)), stream or None))

    def reconstruct_batch_dev(self, d_shards: int, rs: int, bs: int, S: int, nblocks: int,
                              present: Sequence[bool], data_only: bool, stream: int = 0) -> None:
        p = bytearray(1 if x else 0 for x in present)
        _check(lib().rsmi_reconstruct_batch_dev(self._h, d_shards, rs, bs, S, nblocks, ctypes.addressof(_buf(p)),
                                                1 if data_only else 0, stream or None))

    # -- mixed batches: a present (and required) mask per block (rsmi_reconstruct_mixed_*).  A mask
    # argument is nblocks rows of k + m flags (nested sequences, bytes, or a numpy array) or the
    # address of nblocks * (k + m) bytes; required may be None.
    def _masks(self, masks, nblocks: int):
        """(address or None, the object that keeps the bytes alive)."""
        if masks is None:
            return None, None
        if isinstance(masks, int):
            return masks, None
        n = self.k + self.m
        if hasattr(masks, "tobytes"):
            flat = bytearray(masks.tobytes())
        elif isinstance(masks, (bytes, bytearray)):
            flat = bytearray(masks)
        else:
            flat = bytearray(1 if x else 0 for row in masks for x in row)
        if len(flat) != nblocks * n:
            raise RsmiError(ErrInvalidArg, "a mask needs nblocks * (k + m) flags")
        keep = _buf(flat) if flat else None
        return (ctypes.addressof(keep) if flat else None), keep

    def reconstruct_mixed_batch_dev(self, d_shards: int, rs: int, bs: int, S: int, nblocks: int, present,
                                    required=None, data_only: bool = False, stream: int = 0,
                                    status: bool = True) -> Optional[List[int]]:
        """rsmi_reconstruct_mixed_batch_dev.  status: take the per-block statuses (returned as a
        list; blocks with too few rows present are skipped); without it such a block fails the
        whole call with ErrTooFewShards before anything is launched."""
        p, keep_p = self._masks(present, nblocks)
        q, keep_q = self._masks(required, nblocks)
        st = (ctypes.c_int32 * max(nblocks, 1))() if status else None
        _check(lib().rsmi_reconstruct_mixed_batch_dev(self._h, d_shards, rs, bs, S, nblocks, p, q,
                                                      1 if data_only else 0, st, stream or None))
        return list(st)[:nblocks] if status else None

    def reconstruct_mixed_batch_host_ptr(self, ptr: int, bs: int, S: int, nblocks: int, present, required=None,
                                         data_only: bool = False, status: bool = True) -> Optional[List[int]]:
        """rsmi_reconstruct_mixed_batch_host on nblocks blocks of host memory at ptr."""
        p, keep_p = self._masks(present, nblocks)
        q, keep_q = self._masks(required, nblocks)
        st = (ctypes.c_int32 * max(nblocks, 1))() if status else None
        _check(lib().rsmi_reconstruct_mixed_batch_host(self._h, ptr, bs, S, nblocks, p, q, 1 if data_only else 0, st))
        return list(st)[:nblocks] if status else None

    def reconstruct_mixed_batch_dev_crcs(self, d_shards: int, rs: int, bs: int, S: int, nblocks: int, present,
                                         required=None, data_only: bool = False, d_raw16: int = 0, d_raw32: int = 0,
                                         stream: int = 0, status: bool = True) -> Optional[List[int]]:
        """rsmi_reconstruct_mixed_batch_dev_crcs: reconstruct_mixed_batch_dev plus R / R32 of every
        row it rebuilt in d_raw16 / d_raw32[b*(k+m) + r] (uint32, device memory, 0 elsewhere)."""
        p, keep_p = self._masks(present, nblocks)
        q, keep_q = self._masks(required, nblocks)
        st = (ctypes.c_int32 * max(nblocks, 1))() if status else None
        _check(lib().rsmi_reconstruct_mixed_batch_dev_crcs(self._h, d_shards, rs, bs, S, nblocks, p, q,
                                                           1 if data_only else 0, st, d_raw16 or None,
                                                           d_raw32 or None, stream or None))
        return list(st)[:nblocks] if status else None

    def reconstruct_mixed_batch_host_crcs_ptr(self, ptr: int, bs: int, S: int, nblocks: int, present, required=None,
                                              data_only: bool = False, raw16_ptr: Optional[int] = None,
                                              raw32_ptr: Optional[int] = None,
                                              status: bool = True) -> Optional[List[int]]:
        """rsmi_reconstruct_mixed_batch_host_crcs on nblocks blocks of host memory at ptr; the raw
        checksums land in host memory at raw16_ptr / raw32_ptr (nblocks * (k+m) uint32 each)."""
        p, keep_p = self._masks(present, nblocks)
        q, keep_q = self._masks(required, nblocks)
        st = (ctypes.c_int32 * max(nblocks, 1))() if status else None
        _check(lib().rsmi_reconstruct_mixed_batch_host_crcs(self._h, ptr, bs, S, nblocks, p, q, 1 if data_only else 0,
                                                            st, raw16_ptr or None, raw32_ptr or None))
        return list(st)[:nblocks] if status else None

    def reconstruct_mixed_batch_dev_verify(self, d_shards: int, rs: int, bs: int, S: int, nblocks: int, present,
                                           required=None, data_only: bool = False, d_raw16_rows: int = 0,
                                           stream: int = 0, status: bool = True) -> Optional[List[int]]:
        """rsmi_reconstruct_mixed_batch_dev_verify: reconstruct_mixed_batch_dev plus R of every row it
        read (a block's first k present rows) or rebuilt in d_raw16_rows[b*(k+m) + r] (uint32, device
        memory, 0 elsewhere)."""
        p, keep_p = self._masks(present, nblocks)
        q, keep_q = self._masks(required, nblocks)
        st = (ctypes.c_int32 * max(nblocks, 1))() if status else None
        _check(lib().rsmi_reconstruct_mixed_batch_dev_verify(self._h, d_shards, rs, bs, S, nblocks, p, q,
                                                             1 if data_only else 0, st, d_raw16_rows or None,
                                                             stream or None))
        return list(st)[:nblocks] if status else None

    def reconstruct_mixed_batch_host_verify_ptr(self, ptr: int, bs: int, S: int, nblocks: int, present, required=None,
                                                data_only: bool = False, raw16_rows_ptr: Optional[int] = None,
                                                status: bool = True) -> Optional[List[int]]:
        """rsmi_reconstruct_mixed_batch_host_verify on nblocks blocks of host memory at ptr; the raw
        checksums land in host memory at raw16_rows_ptr (nblocks * (k+m) uint32)."""
        p, keep_p = self._masks(present, nblocks)
        q, keep_q = self._masks(required, nblocks)
        st = (ctypes.c_int32 * max(nblocks, 1))() if status else None
        _check(lib().rsmi_reconstruct_mixed_batch_host_verify(self._h, ptr, bs, S, nblocks, p, q,
                                                              1 if data_only else 0, st, raw16_rows_ptr or None))
        return list(st)[:nblocks] if status else None

    def crc_named_rows_dev(self, d_data: int, data_rs: int, data_bs: int, d_parity: int, parity_rs: int,
                           parity_bs: int, S: int, nblocks: int, d_rows: int, slots: int, d_raw16: int = 0,
                           d_raw32: int = 0, stream: int = 0) -> None:
        """rsmi_crc_named_rows_dev: R / R32 of the rows d_rows[b*slots + s] names (int32, device memory;
        heal_batch_dev's d_culprit with slots 1, heal_pair_batch_dev's d_pair with slots 2) in
        d_raw16 / d_raw32[b*slots + s] (uint32, device memory), 0 where an entry names nothing."""
        _check(lib().rsmi_crc_named_rows_dev(self._h, d_data, data_rs, data_bs, d_parity, parity_rs, parity_bs, S,
                                             nblocks, d_rows or None, slots, d_raw16 or None, d_raw32 or None,
                                             stream or None))

    # -- ragged batches: a size and a place per block (rsmi_encode_ragged_*).  blocks is a sequence of
    # (S, data_off, data_shard_stride, parity_off, parity_shard_stride), a numpy array of shape
    # (nblocks, 5) and dtype uint64, a ctypes array of RaggedBlock, or (address, nblocks).
    @staticmethod
    def _ragged(blocks):
        """(address or None, nblocks, the object that keeps the descriptors alive)."""
        if isinstance(blocks, tuple) and len(blocks) == 2 and all(isinstance(x, int) for x in blocks):
            return blocks[0] or None, blocks[1], None
        if isinstance(blocks, ctypes.Array):
            return (ctypes.addressof(blocks) if len(blocks) else None), len(blocks), blocks
        if hasattr(blocks, "ctypes") and hasattr(blocks, "dtype"):
            if blocks.ndim != 2 or blocks.shape[1] != 5 or blocks.dtype.itemsize != 8 or not blocks.flags["C_CONTIGUOUS"]:
                raise RsmiError(ErrInvalidArg, "ragged blocks need a contiguous (nblocks, 5) uint64 array")
            return (blocks.ctypes.data if blocks.shape[0] else None), blocks.shape[0], blocks
        arr = (RaggedBlock * max(len(blocks), 1))()
        for i, b in enumerate(blocks):
            arr[i] = RaggedBlock(*[int(x) for x in b])
        return ctypes.addressof(arr), len(blocks), arr

    def encode_ragged_batch_dev(self, d_data: int, d_parity: int, blocks, stream: int = 0) -> None:
        """rsmi_encode_ragged_batch_dev: the encode of blocks that each have their own shard size and
        rows, device-resident, stream-ordered.  The descriptors are read before the call returns."""
        p, nb, keep = self._ragged(blocks)
        _check(lib().rsmi_encode_ragged_batch_dev(self._h, d_data or None, d_parity or None, p, nb, stream or None))

    def encode_ragged_batch_host_ptr(self, data_ptr: int, parity_ptr: int, blocks) -> None:
        """rsmi_encode_ragged_batch_host: the same descriptors over host bases."""
        p, nb, keep = self._ragged(blocks)
        _check(lib().rsmi_encode_ragged_batch_host(self._h, data_ptr or None, parity_ptr or None, p, nb))

    def encode_ragged_classify(self, data_base: int, parity_base: int, blocks):
        """rsmi_encode_ragged_classify, device-free: (the blocks' classes, Ragged*; their 1 KiB-per-row
        tiles per plan tile, 0 for a fallback block).  The bases count for their alignment only."""
        p, nb, keep = self._ragged(blocks)
        cls = (ctypes.c_uint8 * max(nb, 1))()
        tiles = (ctypes.c_uint64 * max(nb, 1))()
        _check(lib().rsmi_encode_ragged_classify(self._h, data_base or None, parity_base or None, p, nb, cls, tiles))
        return list(cls)[:nb], list(tiles)[:nb]

    def reconstruct_mixed_classify(self, nblocks: int, present, required=None, data_only: bool = False):
        """rsmi_reconstruct_mixed_classify, device-free: (statuses, rows written per block, the
        blocks' pattern indices by first appearance, the number of patterns)."""
        p, keep_p = self._masks(present, nblocks)
        q, keep_q = self._masks(required, nblocks)
        st = (ctypes.c_int32 * max(nblocks, 1))()
        rows = (ctypes.c_uint8 * max(nblocks, 1))()
        pat = (ctypes.c_uint32 * max(nblocks, 1))()
        npat = ctypes.c_size_t(0)
        _check(lib().rsmi_reconstruct_mixed_classify(self._h, nblocks, p, q, 1 if data_only else 0, st, rows, pat,
                                                     ctypes.byref(npat)))
        return list(st)[:nblocks], list(rows)[:nblocks], list(pat)[:nblocks], int(npat.value)


class DeviceGroup:
    """Several GPUs from one process (rsmi_group_open): batches split into contiguous block
    ranges, one per member context, run concurrently (include/rsmi.h "device groups").  The
    reference's Dag Pool runs all its DagNodes in one process (dag/pool/poolservice/cluster.go:
    28-41); members may repeat a device."""

    def __init__(self, k: int, m: int, devices: Sequence[int]):
        arr = (ctypes.c_int * len(devices))(*devices)
        h = ctypes.c_void_p()
        _check(lib().rsmi_group_open(k, m, arr, len(devices), ctypes.byref(h)))
        self.k, self.m, self.n, self.devices = k, m, k + m, list(devices)
        self._h = h

    def close(self) -> None:
        if self._h:
            lib().rsmi_group_close(self._h)
            self._h = ctypes.c_void_p()

    def __del__(self):  # pragma: no cover
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def size(self) -> int:
        return lib().rsmi_group_size(self._h)

    def member_of_key(self, key: bytes) -> int:
        b = bytearray(key)
        return lib().rsmi_group_member_of_key(self._h, ctypes.addressof(_buf(b)) if b else None, len(b))

    def member_numa_node(self, i: int) -> int:
        return lib().rsmi_group_member_numa_node(self._h, i)

    def host_alloc(self, block_bytes: int, nblocks: int) -> int:
        """Page-locked buffer whose member block ranges sit on the members' NUMA nodes."""
        p = lib().rsmi_group_host_alloc(self._h, block_bytes, nblocks)
        if not p:  # mmap, NUMA placement or page-locking the host range failed
            raise RsmiError(ErrHost, "rsmi_group_host_alloc failed")
        return p

    def host_free(self, p: int) -> None:
        lib().rsmi_group_host_free(self._h, p)

    def encode_batch_host_ptr(self, data_ptr: int, data_bs: int, parity_ptr: int, parity_bs: int, S: int,
                              nblocks: int) -> None:
        _check(lib().rsmi_group_encode_batch_host(self._h, data_ptr, data_bs, parity_ptr, parity_bs, S, nblocks))

    def encode_batch_host_crcs_ptr(self, data_ptr: int, data_bs: int, parity_ptr: int, parity_bs: int, S: int,
                                   nblocks: int, raw16_ptr: Optional[int], raw32_ptr: Optional[int]) -> None:
        _check(lib().rsmi_group_encode_batch_host_crcs(self._h, data_ptr, data_bs, parity_ptr, parity_bs, S, nblocks,
                                                     raw16_ptr or None, raw32_ptr or None))

    def reconstruct_batch_host_ptr(self, ptr: int, bs: int, S: int, nblocks: int, present: Sequence[bool],
                                   data_only: bool) -> None:
        p = bytearray(1 if x else 0 for x in present)
        _check(lib().rsmi_group_reconstruct_batch_host(self._h, ptr, bs, S, nblocks, ctypes.addressof(_buf(p)),
                                                     1 if data_only else 0))

    def reconstruct_rows_batch_host_ptr(self, ptr: int, bs: int, S: int, nblocks: int, present: Sequence[bool],
                                        required: Sequence[bool]) -> None:
        p = bytearray(1 if x else 0 for x in present)
        q = bytearray(1 if x else 0 for x in required)
        _check(lib().rsmi_group_reconstruct_rows_batch_host(self._h, ptr, bs, S, nblocks, ctypes.addressof(_buf(p)),
                                                          ctypes.addressof(_buf(q))))


def device_numa_node(device: int) -> int:
    return lib().rsmi_device_numa_node(device)


def sysfs_numa_node(sysfs_root: str, pci_bus_id: str) -> int:
    return lib().rsmi_sysfs_numa_node(sysfs_root.encode(), pci_bus_id.encode())


def sysfs_node_cpus(sysfs_root: str, node: int) -> Optional[list]:
    """CPU ids of a NUMA node from <sysfs_root>/devices/system/node/node<N>/cpulist (None if absent)."""
    L = lib()
    n = L.rsmi_sysfs_node_cpus(sysfs_root.encode(), node, None, 0)
    if n < 0:
        return None
    arr = (ctypes.c_int * max(n, 1))()
    L.rsmi_sysfs_node_cpus(sysfs_root.encode(), node, arr, n)
    return list(arr[:n])


def partition(nblocks: int, parts: int, i: int):
    """rsmi_partition: (start, count) of member i's contiguous range."""
    st, cnt = ctypes.c_size_t(), ctypes.c_size_t()
    _check(lib().rsmi_partition(nblocks, parts, i, ctypes.byref(st), ctypes.byref(cnt)))
    return st.value, cnt.value


def key_slot(key: bytes) -> int:
    """keyHashSlot (dag/pool/poolservice/hash_slot.go:20-22) in the library."""
    b = bytearray(key)
    return lib().rsmi_key_slot(ctypes.addressof(_buf(b)) if b else None, len(b))


def check_shards(lens: Sequence[int], nil_ok: bool):
    arr = (ctypes.c_size_t * len(lens))(*lens)
    S = ctypes.c_size_t()
    rc = lib().rsmi_check_shards(len(lens), arr, 1 if nil_ok else 0, ctypes.byref(S))
    return rc, S.value


class Erasure:
    """dag/node/dagnode/erasure.go:9-13 Erasure{encoder, dataBlocks, parityBlocks, blockSize}."""

    def __init__(self, data_blocks: int, parity_blocks: int, block_size: int, device: int = 0):
        # erasure.go:18-24
        if data_blocks <= 0 or parity_blocks <= 0:
            raise RsmiError(ErrInvShardNum)
        if data_blocks + parity_blocks > 256:
            raise RsmiError(ErrMaxShardNum)
        self.data_blocks = data_blocks
        self.parity_blocks = parity_blocks
        self.block_size = block_size
        self._device = device
        self._codec: Optional[Codec] = None

    def encoder(self) -> Codec:
        """erasure.go:31-45: the codec is built lazily, once."""
        if self._codec is None:
            self._codec = Codec(self.data_blocks, self.parity_blocks, self._device)
        return self._codec

    def shard_size(self) -> int:
        """erasure.go:96-98"""
        return ceil_frac(self.block_size, self.data_blocks)

    def encode_data(self, data: bytes) -> List[Optional[bytes]]:
        """erasure.go:51-65 EncodeData: Split + Encode."""
        n = self.data_blocks + self.parity_blocks
        if len(data) == 0:
            return [None] * n
        flat = self.encoder().encode_block(data)
        S = len(flat) // n
        return [flat[i * S:(i + 1) * S] for i in range(n)]

    def encode_data_many(self, blocks: List[bytes]) -> List[List[Optional[bytes]]]:
        """encode_data for many blocks at once, each of its own length, through one
        rsmi_encode_ragged_batch_host call: the result equals [encode_data(b) for b in blocks] (an
        empty block gives k + m times None, as there).  The Split of every non-empty block (shard
        size ceilFrac(len, k), the last data shards zero-padded) is done here into one buffer, a
        block's k + m rows side by side at pitch roundup(S, 16)."""
        k, n = self.data_blocks, self.data_blocks + self.parity_blocks
        out: List[List[Optional[bytes]]] = [[None] * n for _ in blocks]
        work = []  # (block index, S, pitch, offset of the block's rows)
        total = 0
        for bi, data in enumerate(blocks):
            if len(data) == 0:
                continue
            S = ceil_frac(len(data), k)
            P = (S + 15) // 16 * 16
            work.append((bi, S, P, total))
            total += n * P
        if not work:
            return out
        flat = bytearray(total)
        for bi, S, P, off in work:
            data = blocks[bi]
            for i in range(k):
                row = data[i * S:(i + 1) * S]
                flat[off + i * P:off + i * P + len(row)] = row
        desc = (RaggedBlock * len(work))()
        for j, (bi, S, P, off) in enumerate(work):
            desc[j] = RaggedBlock(S, off, P, off + k * P, P)
        base = ctypes.addressof(_buf(flat))
        self.encoder().encode_ragged_batch_host_ptr(base, base, desc)
        for bi, S, P, off in work:
            out[bi] = [bytes(flat[off + i * P:off + i * P + S]) for i in range(n)]
        return out

    def _reconstruct(self, shards: List[Optional[bytes]], data_only: bool) -> None:
        n = self.data_blocks + self.parity_blocks
        if len(shards) != n:
            raise RsmiError(ErrTooFewShards)  # upstream: len(shards) != totalShards
        lens = [len(s) if s else 0 for s in shards]
        rc, S = check_shards(lens, nil_ok=True)
        _check(rc)
        present = [bool(x) for x in lens]
        np_ = sum(present)
        dp = sum(present[: self.data_blocks])
        if np_ == n or (data_only and dp == self.data_blocks):
            return
        flat = bytearray(n * S)
        for i, s in enumerate(shards):
            if s:
                flat[i * S:(i + 1) * S] = s
        self.encoder().reconstruct(flat, S, present, data_only)
        for i in range(n):
            if not present[i] and (i < self.data_blocks or not data_only):
                shards[i] = bytes(flat[i * S:(i + 1) * S])

    def decode_data_blocks(self, data: List[Optional[bytes]]) -> None:
        """erasure.go:70-83 DecodeDataBlocks (the isZero loop breaks after the first empty
        shard, so only 'nothing missing' short-circuits; then ReconstructData)."""
        is_zero = 0
        for b in data:
            if not b:
                is_zero += 1
                break
        if is_zero == 0 or is_zero == len(data):
            return
        self._reconstruct(data, data_only=True)

    def decode_data_blocks_many(self, blocks: List[List[Optional[bytes]]]) -> None:
        """decode_data_blocks for many blocks at once, each with its own missing shards, through
        one rsmi_reconstruct_mixed_batch_host call.  Every block passes decode_data_blocks' checks
        first, in order (the isZero loop, the shard count, checkShards, nothing missing, fewer than
        k shards present); when a block fails one, the first such block's sentinel is raised before
        anything is decoded, and no list is changed.  Blocks that need decoding must share one
        shard size (ErrShardSize at the first that differs).  The missing data shards of every
        block are then filled in place, as decode_data_blocks fills them."""
        k, n = self.data_blocks, self.data_blocks + self.parity_blocks
        work = []  # (block index, present flags)
        S = 0
        for bi, data in enumerate(blocks):
            if all(data) or len(data) == 1:  # decode_data_blocks' isZero short-circuit
                continue
            if len(data) != n:
                raise RsmiError(ErrTooFewShards)
            rc, s = check_shards([len(x) if x else 0 for x in data], nil_ok=True)
            _check(rc)
            present = [bool(x) for x in data]
            if sum(present[:k]) == k:
                continue
            if sum(present) < k:
                raise RsmiError(ErrTooFewShards)
            if work and s != S:
                raise RsmiError(ErrShardSize)
            S = s
            work.append((bi, present))
        if not work:
            return
        flat = bytearray(len(work) * n * S)
        for j, (bi, present) in enumerate(work):
            for i, x in enumerate(blocks[bi]):
                if x:
                    flat[(j * n + i) * S:(j * n + i + 1) * S] = x
        status = self.encoder().reconstruct_mixed_batch_host_ptr(
            ctypes.addressof(_buf(flat)), n * S, S, len(work), [p for _, p in work], None, True)
        for st in status:
            _check(st)
        for j, (bi, present) in enumerate(work):
            for i in range(k):
                if not present[i]:
                    blocks[bi][i] = bytes(flat[(j * n + i) * S:(j * n + i + 1) * S])

    def decode_data_and_parity_blocks(self, data: List[Optional[bytes]]) -> None:
        """erasure.go:87-93 DecodeDataAndParityBlocks -> Reconstruct."""
        self._reconstruct(data, data_only=False)

    def verify(self, shards: List[bytes]) -> bool:
        """Encoder.Verify (not called by erasure.go; offered for scrubs): True iff the parity
        shards are the encode of the data shards.  Upstream's checks come first: a shard list of
        the wrong length is ErrTooFewShards, and checkShards with nilok = false rejects empty
        lists (ErrShardNoData) and missing or unequal shards (ErrShardSize)."""
        n = self.data_blocks + self.parity_blocks
        if len(shards) != n:
            raise RsmiError(ErrTooFewShards)  # upstream: len(shards) != totalShards
        rc, S = check_shards([len(s) if s else 0 for s in shards], nil_ok=False)
        _check(rc)
        return self.encoder().verify(bytearray(b"".join(shards)), S)

    def scrub(self, shards: List[bytes]) -> Tuple[bool, List[int]]:
        """The first pass of a scrub (rsmi_scrub): (verify's answer, R(shard) of every shard as
        stored, ready for crc16_entry), from one read of the shards.  The shard list is checked as
        verify checks it."""
        n = self.data_blocks + self.parity_blocks
        if len(shards) != n:
            raise RsmiError(ErrTooFewShards)
        rc, S = check_shards([len(s) if s else 0 for s in shards], nil_ok=False)
        _check(rc)
        return self.encoder().scrub(bytearray(b"".join(shards)), S)

    def locate(self, shards: List[bytes]) -> int:
        """Which shard breaks the stripe (rsmi_locate): LocateClean, the index of the one shard
        whose replacement by its reconstruction makes the stripe clean, or LocateUnknown.  The
        shard list is checked as verify checks it."""
        n = self.data_blocks + self.parity_blocks
        if len(shards) != n:
            raise RsmiError(ErrTooFewShards)
        rc, S = check_shards([len(s) if s else 0 for s in shards], nil_ok=False)
        _check(rc)
        return self.encoder().locate(bytearray(b"".join(shards)), S)

    def locate_pair(self, shards: List[bytes]) -> Tuple[int, int]:
        """Which shards break the stripe (rsmi_locate_pair): (-1, -1) clean, (x, -1) locate's single
        shard, (x, y) the one pair whose replacement by its reconstruction makes the stripe clean,
        or (-2, -2).  The shard list is checked as verify checks it."""
        n = self.data_blocks + self.parity_blocks
        if len(shards) != n:
            raise RsmiError(ErrTooFewShards)
        rc, S = check_shards([len(s) if s else 0 for s in shards], nil_ok=False)
        _check(rc)
        return self.encoder().locate_pair(bytearray(b"".join(shards)), S)

    def heal(self, shards: List[bytes]) -> Tuple[int, List[bytes]]:
        """Locate, then rewrite the named shard (rsmi_heal): (verdict, shards), the verdict that of
        locate for the list as given; when it names a shard, that entry of the returned list is
        its reconstruction from the others, every other entry is the caller's.  The shard list is
        checked as verify checks it."""
        n = self.data_blocks + self.parity_blocks
        if len(shards) != n:
            raise RsmiError(ErrTooFewShards)
        rc, S = check_shards([len(s) if s else 0 for s in shards], nil_ok=False)
        _check(rc)
        buf = bytearray(b"".join(shards))
        v = self.encoder().heal(buf, S)
        out = list(shards)
        if v >= 0:
            out[v] = bytes(buf[v * S:(v + 1) * S])
        return v, out

    def heal_pair(self, shards: List[bytes]) -> Tuple[Tuple[int, int], List[bytes]]:
        """Locate singles and pairs, then rewrite the named shards (rsmi_heal_pair): ((x, y), shards),
        the verdict that of locate_pair for the list as given; the entries it names are their
        reconstruction from the others, every other entry is the caller's.  The shard list is
        checked as verify checks it."""
        n = self.data_blocks + self.parity_blocks
        if len(shards) != n:
            raise RsmiError(ErrTooFewShards)
        rc, S = check_shards([len(s) if s else 0 for s in shards], nil_ok=False)
        _check(rc)
        buf = bytearray(b"".join(shards))
        v = self.encoder().heal_pair(buf, S)
        out = list(shards)
        for x in v:
            if x >= 0:
                out[x] = bytes(buf[x * S:(x + 1) * S])
        return v, out


def NewErasure(data_blocks: int, parity_blocks: int, block_size: int, device: int = 0) -> Erasure:
    return Erasure(data_blocks, parity_blocks, block_size, device)


def crc16_ibm(data: bytes) -> int:
    """howeyc/crc16 Checksum(data, IBMTable) (dag/node/datanode/server.go:70), host side."""
    b = bytearray(data)
    return lib().rsmi_crc16_ibm(ctypes.addressof(_buf(b)) if b else None, len(b))


def crc16_entry(head: bytes, raw: int, data_len: int) -> int:
    """Checksum(head || D) from R(D) = raw and |D| (include/rsmi.h rsmi_crc16_entry)."""
    h = bytearray(head)
    return lib().rsmi_crc16_entry(ctypes.addressof(_buf(h)) if h else None, len(h), raw, data_len)


def crc32_ieee(data: bytes) -> int:
    """Go crc32.ChecksumIEEE(data) (the mutcask value checksum, kv/mutcask/cask.go:75), host side."""
    b = bytearray(data)
    return lib().rsmi_crc32_ieee(ctypes.addressof(_buf(b)) if b else None, len(b))


def crc32_entry(head: bytes, raw: int, data_len: int) -> int:
    """ChecksumIEEE(head || D) from R32(D) = raw and |D| (include/rsmi.h rsmi_crc32_entry)."""
    h = bytearray(head)
    return lib().rsmi_crc32_entry(ctypes.addressof(_buf(h)) if h else None, len(h), raw, data_len)


def recommended_pitch(S: int) -> int:
    return lib().rsmi_recommended_pitch(S)


def device_count() -> int:
    return lib().rsmi_device_count()
