"""ctypes binding of libcarbonado_hip.so (include/carbonado_hip.h).

The shared library is the product: HIP kernels for gfx950 behind a C-ABI.
This module only loads it and declares signatures.  There is no fallback:
if the library is missing, or no gfx950 device is visible, compute calls
raise instead of silently running elsewhere.
"""
from __future__ import annotations

import ctypes
import os
from pathlib import Path

# CARBONADO_HIP_LIB: another build of the same library (A/B calibration tools only)
LIB_PATH = Path(os.environ.get("CARBONADO_HIP_LIB") or Path(__file__).resolve().parent / "lib" / "libcarbonado_hip.so")

c_u8p = ctypes.POINTER(ctypes.c_uint8)
c_u32p = ctypes.POINTER(ctypes.c_uint32)
c_u64p = ctypes.POINTER(ctypes.c_uint64)


class EncodeInfoC(ctypes.Structure):
    """chip_encode_info == structs.rs:12-44 EncodeInfo, field for field."""

    _fields_ = [
        ("input_len", ctypes.c_uint32),
        ("output_len", ctypes.c_uint32),
        ("bytes_compressed", ctypes.c_uint32),
        ("compression_factor", ctypes.c_float),
        ("bytes_encrypted", ctypes.c_uint32),
        ("bytes_ecc", ctypes.c_uint32),
        ("bytes_verifiable", ctypes.c_uint32),
        ("amplification_factor", ctypes.c_float),
        ("padding_len", ctypes.c_uint32),
        ("chunk_len", ctypes.c_uint32),
        ("verifiable_slice_count", ctypes.c_uint16),
        ("chunk_slice_count", ctypes.c_uint16),
    ]


class EciesInjectC(ctypes.Structure):
    """chip_ecies_inject: the values ecies::encrypt draws from thread_rng."""

    _fields_ = [("ephemeral_sk", ctypes.c_void_p), ("nonce", ctypes.c_void_p)]


class HeaderC(ctypes.Structure):
    """chip_header == file.rs:24-43 Header, deserialized."""

    _fields_ = [
        ("pubkey", ctypes.c_uint8 * 33),
        ("hash", ctypes.c_uint8 * 32),
        ("signature", ctypes.c_uint8 * 64),
        ("format", ctypes.c_uint8),
        ("chunk_index", ctypes.c_uint8),
        ("encoded_len", ctypes.c_uint32),
        ("padding_len", ctypes.c_uint32),
        ("metadata", ctypes.c_uint8 * 8),
        ("has_metadata", ctypes.c_uint8),
    ]


# name -> (restype, argtypes); mirrors include/carbonado_hip.h exactly
SIGNATURES = {
    "chip_abi_version": (ctypes.c_int, []),
    "chip_strerror": (ctypes.c_char_p, [ctypes.c_int]),
    "chip_init": (ctypes.c_int, [ctypes.c_int]),
    "chip_last_device_error": (ctypes.c_char_p, []),
    "chip_device_alloc": (ctypes.c_int, [ctypes.c_uint64, ctypes.POINTER(ctypes.c_void_p)]),
    "chip_device_free": (ctypes.c_int, [ctypes.c_void_p]),
    "chip_schnorr_sign": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_uint64, ctypes.c_void_p, ctypes.c_void_p,
                                         ctypes.c_void_p]),
    "chip_schnorr_verify": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_uint64, ctypes.c_void_p, ctypes.c_void_p]),
    "chip_header_new": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_uint64, ctypes.c_void_p, ctypes.c_uint64,
                                       ctypes.c_void_p, ctypes.c_uint64, ctypes.c_uint8, ctypes.c_uint8,
                                       ctypes.c_uint32, ctypes.c_uint32, ctypes.c_void_p, ctypes.c_void_p,
                                       ctypes.POINTER(HeaderC)]),
    "chip_header_to_bytes": (ctypes.c_int, [ctypes.POINTER(HeaderC), ctypes.c_void_p]),
    "chip_header_parse": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_uint64, ctypes.POINTER(HeaderC)]),
    "chip_file_encode": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_uint64, ctypes.c_void_p, ctypes.c_uint64,
                                        ctypes.c_void_p, ctypes.c_uint64, ctypes.c_uint8, ctypes.c_void_p,
                                        ctypes.POINTER(EciesInjectC), ctypes.c_void_p, ctypes.c_void_p,
                                        ctypes.c_uint64, c_u64p, ctypes.POINTER(EncodeInfoC)]),
    "chip_file_decode": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_uint64, ctypes.c_void_p, ctypes.c_uint64,
                                        ctypes.POINTER(HeaderC), ctypes.c_void_p, ctypes.c_uint64, c_u64p]),
    "chip_device_alloc_info": (ctypes.c_int, [ctypes.c_void_p, ctypes.POINTER(ctypes.c_uint32),
                                              ctypes.POINTER(ctypes.c_uint32), ctypes.POINTER(ctypes.c_double)]),
    "chip_stream_queue_block": (ctypes.c_int, [ctypes.c_void_p, ctypes.POINTER(ctypes.c_uint64)]),
    "chip_host_topology": (ctypes.c_int, [ctypes.c_char_p, ctypes.c_uint64, ctypes.POINTER(ctypes.c_uint64)]),
    "chip_torch_alloc": (ctypes.c_void_p, [ctypes.c_ssize_t, ctypes.c_int, ctypes.c_void_p]),
    "chip_torch_free": (None, [ctypes.c_void_p, ctypes.c_ssize_t, ctypes.c_int, ctypes.c_void_p]),
    "chip_calc_padding_len": (ctypes.c_int, [ctypes.c_uint64, ctypes.c_uint32, c_u32p, c_u32p]),
    "chip_zfec_encoded_len": (ctypes.c_uint64, [ctypes.c_uint64, ctypes.c_uint32, ctypes.c_uint32]),
    "chip_bao_encoded_len": (ctypes.c_uint64, [ctypes.c_uint64]),
    "chip_encode_max_len": (ctypes.c_uint64, [ctypes.c_uint64]),
    "chip_zfec_encode": (ctypes.c_int, [ctypes.c_uint32, ctypes.c_uint32, ctypes.c_void_p, ctypes.c_uint64,
                                        ctypes.c_void_p, ctypes.c_uint64, c_u32p, c_u32p]),
    "chip_zfec_decode": (ctypes.c_int, [ctypes.c_uint32, ctypes.c_uint32, ctypes.c_void_p, ctypes.c_uint64,
                                        ctypes.c_uint32, ctypes.c_void_p, ctypes.c_uint64, c_u64p]),
    "chip_zfec_decode_shares": (ctypes.c_int, [ctypes.c_uint32, ctypes.c_uint32,
                                               ctypes.POINTER(ctypes.c_void_p), c_u32p, ctypes.c_uint32,
                                               ctypes.c_uint64, ctypes.c_uint32, ctypes.c_void_p,
                                               ctypes.c_uint64, c_u64p]),
    "chip_bao_encode": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_uint64, ctypes.c_void_p, ctypes.c_uint64,
                                       c_u64p, ctypes.c_void_p]),
    "chip_bao_decode": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_uint64, ctypes.c_void_p, ctypes.c_uint64,
                                       ctypes.c_void_p, ctypes.c_uint64, c_u64p]),
    "chip_blake3": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_uint64, ctypes.c_void_p]),
    "chip_snap_max_len": (ctypes.c_uint64, [ctypes.c_uint64]),
    "chip_snap_compress": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_uint64, ctypes.c_void_p, ctypes.c_uint64,
                                          c_u64p]),
    "chip_snap_decompress": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_uint64, ctypes.c_void_p, ctypes.c_uint64,
                                            c_u64p]),
    "chip_ecies_encrypt": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_uint64, ctypes.POINTER(EciesInjectC),
                                          ctypes.c_void_p, ctypes.c_uint64, ctypes.c_void_p, ctypes.c_uint64,
                                          c_u64p]),
    "chip_ecies_decrypt": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_uint64, ctypes.c_void_p, ctypes.c_uint64,
                                          ctypes.c_void_p, ctypes.c_uint64, c_u64p]),
    "chip_ecies_public_key": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p]),
    "chip_encode": (ctypes.c_int, [ctypes.c_uint8, ctypes.c_void_p, ctypes.c_uint64, ctypes.POINTER(EciesInjectC),
                                   ctypes.c_void_p, ctypes.c_uint64, ctypes.c_void_p, ctypes.c_uint64, c_u64p,
                                   ctypes.c_void_p, ctypes.POINTER(EncodeInfoC)]),
    "chip_decode": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_uint64, ctypes.c_void_p, ctypes.c_uint64,
                                   ctypes.c_void_p, ctypes.c_uint64, ctypes.c_uint32, ctypes.c_uint8,
                                   ctypes.c_void_p, ctypes.c_uint64, c_u64p]),
    "chip_zfec_encode_batch_dev": (ctypes.c_int, [ctypes.c_uint32, ctypes.c_uint32, ctypes.c_void_p,
                                                  ctypes.c_uint64, ctypes.c_uint64, ctypes.c_uint64,
                                                  ctypes.c_void_p, ctypes.c_uint64, ctypes.c_void_p]),
    "chip_hbm_pattern_batch_dev": (ctypes.c_int, [ctypes.c_uint32, ctypes.c_uint32, ctypes.c_void_p,
                                                  ctypes.c_uint64, ctypes.c_uint64, ctypes.c_uint64,
                                                  ctypes.c_void_p, ctypes.c_uint64, ctypes.c_void_p]),
    "chip_zfec_decode_batch_dev": (ctypes.c_int, [ctypes.c_uint32, ctypes.c_uint32, ctypes.c_void_p,
                                                  ctypes.c_uint64, ctypes.c_uint64, c_u32p, ctypes.c_uint32,
                                                  ctypes.c_uint64, ctypes.c_void_p, ctypes.c_uint64,
                                                  ctypes.c_void_p]),
    "chip_bao_scratch_len": (ctypes.c_uint64, [ctypes.c_uint64, ctypes.c_uint64]),
    "chip_bao_encode_batch_dev": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_uint64, ctypes.c_uint64,
                                                 ctypes.c_uint64, ctypes.c_void_p, ctypes.c_uint64,
                                                 ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]),
    "chip_bao_decode_batch_dev": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_uint64, ctypes.c_uint64,
                                                 ctypes.c_uint64, ctypes.c_void_p, ctypes.c_void_p,
                                                 ctypes.c_uint64, ctypes.c_void_p, ctypes.c_void_p,
                                                 ctypes.c_void_p]),
    "chip_encode_scratch_len": (ctypes.c_uint64, [ctypes.c_uint8, ctypes.c_uint64, ctypes.c_uint64]),
    "chip_encode_batch_dev": (ctypes.c_int, [ctypes.c_uint8, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_uint64,
                                             ctypes.c_uint64, ctypes.c_void_p, ctypes.c_uint64, c_u64p,
                                             ctypes.c_void_p, ctypes.POINTER(EncodeInfoC), ctypes.c_void_p,
                                             ctypes.c_void_p]),
    "chip_decode_scratch_len": (ctypes.c_uint64, [ctypes.c_uint8, ctypes.c_uint64, ctypes.c_uint64]),
    "chip_decode_batch_dev": (ctypes.c_int, [ctypes.c_uint8, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_uint64,
                                             ctypes.c_uint64, ctypes.c_void_p, ctypes.c_uint32, ctypes.c_void_p,
                                             ctypes.c_uint64, c_u64p, ctypes.c_void_p, ctypes.c_void_p,
                                             ctypes.c_void_p]),
    "chip_bao_slice_len": (ctypes.c_uint64, [ctypes.c_uint64, ctypes.c_uint64, ctypes.c_uint64]),
    "chip_bao_extract_slice": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_uint64, ctypes.c_uint64, ctypes.c_uint64,
                                              ctypes.c_void_p, ctypes.c_uint64, c_u64p]),
    "chip_bao_verify_slice": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_uint64, ctypes.c_void_p, ctypes.c_uint64,
                                             ctypes.c_uint64, ctypes.c_uint64, ctypes.c_void_p, ctypes.c_uint64,
                                             c_u64p]),
    "chip_scrub": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_uint64, ctypes.c_void_p, ctypes.c_uint64,
                                  ctypes.c_uint32, ctypes.c_uint32, ctypes.c_void_p, ctypes.c_uint64, c_u64p]),
    "chip_scrub_scratch_len": (ctypes.c_uint64, [ctypes.c_uint64, ctypes.c_uint64]),
    "chip_scrub_batch_dev": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_uint64, ctypes.c_uint64, ctypes.c_uint64,
                                            ctypes.c_void_p, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_void_p,
                                            ctypes.c_uint64, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]),
    "chip_bao_hasher_new": (ctypes.c_int, [ctypes.POINTER(ctypes.c_void_p)]),
    "chip_bao_hasher_update": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint64]),
    "chip_bao_hasher_finalize": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p]),
    "chip_bao_hasher_len": (ctypes.c_uint64, [ctypes.c_void_p]),
    "chip_bao_hasher_read_all": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint64, c_u64p]),
    "chip_bao_hasher_free": (None, [ctypes.c_void_p]),
    "chip_bao_hasher_drop_cache": (ctypes.c_uint64, []),
    "chip_bao_hasher_cached_bytes": (ctypes.c_uint64, []),
    "chip_decode_host_batch": (ctypes.c_int, [ctypes.c_uint8, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_void_p,
                                              ctypes.c_void_p, c_u64p, ctypes.c_uint64, ctypes.c_uint64, c_u32p,
                                              ctypes.c_void_p, ctypes.c_uint64, c_u64p,
                                              ctypes.POINTER(ctypes.c_int32), ctypes.c_uint32, ctypes.c_uint64,
                                              ctypes.c_uint32]),
    "chip_encode_host_batch": (ctypes.c_int, [ctypes.c_uint8, ctypes.c_void_p, ctypes.c_uint64,
                                              ctypes.POINTER(EciesInjectC), ctypes.c_void_p, ctypes.c_uint64,
                                              ctypes.c_uint64, ctypes.c_uint64, ctypes.c_void_p, ctypes.c_uint64,
                                              c_u64p, ctypes.c_void_p, ctypes.POINTER(EncodeInfoC),
                                              ctypes.c_uint32, ctypes.c_uint64, ctypes.c_uint32]),
}

# the extension header (include/carbonado_hip_ext.h): a table of its own, the
# drop-in boundary above stays as it is
EXT_SIGNATURES = {
    "chipx_abi_version": (ctypes.c_int, []),
    "chipx_ragged_layout": (ctypes.c_int, [ctypes.c_uint8, c_u64p, ctypes.c_uint64, ctypes.c_uint64,
                                           ctypes.c_uint64, c_u64p, c_u64p, c_u64p]),
    "chipx_ragged_scratch_len": (ctypes.c_uint64, [ctypes.c_uint8, c_u64p, ctypes.c_uint64, ctypes.c_int]),
    "chipx_encode_ragged_dev": (ctypes.c_int, [ctypes.c_uint8, ctypes.c_void_p, c_u64p, c_u64p, ctypes.c_uint64,
                                               ctypes.c_void_p, c_u64p, c_u64p, ctypes.c_void_p,
                                               ctypes.POINTER(EncodeInfoC), ctypes.c_void_p, ctypes.c_void_p]),
    "chipx_decode_ragged_dev": (ctypes.c_int, [ctypes.c_uint8, ctypes.c_void_p, c_u64p, c_u64p, ctypes.c_uint64,
                                               ctypes.c_void_p, c_u32p, ctypes.c_void_p, c_u64p, c_u64p,
                                               ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]),
}

# the audit header (include/carbonado_hip_audit.h): slice audits of
# device-resident streams, again a table of its own
AUDIT_SIGNATURES = {
    "chipa_abi_version": (ctypes.c_int, []),
    "chipa_slice_layout": (ctypes.c_int, [c_u64p, c_u64p, c_u64p, ctypes.c_uint64, ctypes.c_uint64, c_u64p, c_u64p,
                                          c_u64p, c_u64p, c_u64p, c_u64p]),
    "chipa_audit_scratch_len": (ctypes.c_uint64, [ctypes.c_uint64, ctypes.c_uint64]),
    "chipa_extract_slices_dev": (ctypes.c_int, [ctypes.c_void_p, c_u64p, c_u64p, ctypes.c_uint64, c_u32p, c_u64p,
                                                c_u64p, ctypes.c_uint64, ctypes.c_void_p, c_u64p, c_u64p,
                                                ctypes.c_void_p, ctypes.c_void_p]),
    "chipa_verify_slices_dev": (ctypes.c_int, [ctypes.c_void_p, c_u64p, c_u64p, ctypes.c_void_p, ctypes.c_uint64,
                                               c_u32p, c_u64p, c_u64p, ctypes.c_uint64, ctypes.c_void_p, c_u64p,
                                               c_u64p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]),
    "chipa_verify_proofs_dev": (ctypes.c_int, [ctypes.c_void_p, c_u64p, c_u64p, c_u64p, ctypes.c_void_p, c_u64p,
                                               c_u64p, ctypes.c_uint64, ctypes.c_void_p, c_u64p, c_u64p,
                                               ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]),
}

# the repair header (include/carbonado_hip_repair.h): the ragged scrub of
# device-resident Bao|Zfec streams, a fourth table of its own
REPAIR_SIGNATURES = {
    "chipr_abi_version": (ctypes.c_int, []),
    "chipr_scrub_ragged_scratch_len": (ctypes.c_uint64, [c_u64p, ctypes.c_uint64, ctypes.c_uint64]),
    "chipr_shard_masks_ragged_dev": (ctypes.c_int, [ctypes.c_void_p, c_u64p, c_u64p, ctypes.c_uint64, ctypes.c_void_p,
                                                    c_u32p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint64,
                                                    ctypes.c_void_p]),
    "chipr_scrub_ragged_dev": (ctypes.c_int, [ctypes.c_void_p, c_u64p, c_u64p, ctypes.c_uint64, ctypes.c_void_p, c_u32p,
                                              c_u32p, ctypes.c_void_p, c_u64p, ctypes.c_void_p, ctypes.c_void_p,
                                              ctypes.c_uint64, ctypes.c_void_p]),
}

# the read header (include/carbonado_hip_read.h): ranged reads of resident
# Zfec|Bao objects that survive shard damage, a fifth table of its own
READ_SIGNATURES = {
    "chipd_abi_version": (ctypes.c_int, []),
    "chipd_read_layout": (ctypes.c_int, [c_u32p, c_u32p, ctypes.c_uint64, c_u32p, c_u64p, c_u64p, ctypes.c_uint64,
                                         ctypes.c_uint64, c_u64p, c_u64p, c_u64p, c_u64p]),
    "chipd_read_scratch_len": (ctypes.c_uint64, [ctypes.c_uint64, ctypes.c_uint64]),
    "chipd_read_ranges_dev": (ctypes.c_int, [ctypes.c_void_p, c_u64p, c_u64p, ctypes.c_void_p, c_u32p, c_u32p,
                                             ctypes.c_uint64, c_u32p, c_u64p, c_u64p, ctypes.c_uint64, ctypes.c_void_p,
                                             c_u64p, c_u64p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
                                             ctypes.c_uint64, ctypes.c_void_p]),
}

# the vread header (include/carbonado_hip_vread.h): ranged reads whose rebuilt
# chunks are hashed against the stored tree, a sixth table of its own
VREAD_SIGNATURES = {
    "chipv_abi_version": (ctypes.c_int, []),
    "chipv_read_scratch_len": (ctypes.c_uint64, [ctypes.c_uint64, ctypes.c_uint64]),
    "chipv_read_ranges_dev": (ctypes.c_int, [ctypes.c_void_p, c_u64p, c_u64p, ctypes.c_void_p, c_u32p, c_u32p,
                                             ctypes.c_uint64, c_u32p, c_u64p, c_u64p, ctypes.c_uint64, ctypes.c_void_p,
                                             c_u64p, c_u64p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
                                             ctypes.c_uint32, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_void_p]),
}

# the ecies header (include/carbonado_hip_ecies.h): AES-256-GCM over resident
# messages, a seventh table of its own
ECIES_SIGNATURES = {
    "chipe_abi_version": (ctypes.c_int, []),
    "chipe_gcm_scratch_len": (ctypes.c_uint64, [c_u64p, ctypes.c_uint64]),
    "chipe_gcm_seal_ragged_dev": (ctypes.c_int, [c_u8p, c_u8p, ctypes.c_void_p, c_u64p, c_u64p, ctypes.c_uint64,
                                                 ctypes.c_void_p, c_u64p, ctypes.c_void_p, ctypes.c_void_p,
                                                 ctypes.c_uint64, ctypes.c_void_p]),
    "chipe_gcm_open_ragged_dev": (ctypes.c_int, [c_u8p, c_u8p, ctypes.c_void_p, c_u64p, c_u64p, ctypes.c_uint64,
                                                 ctypes.c_void_p, ctypes.c_void_p, c_u64p, ctypes.c_void_p,
                                                 ctypes.c_void_p, ctypes.c_uint64, ctypes.c_void_p]),
    "chipe_seal_ragged_dev": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_uint64, ctypes.POINTER(EciesInjectC),
                                             ctypes.c_void_p, c_u64p, c_u64p, ctypes.c_uint64, ctypes.c_void_p,
                                             c_u64p, ctypes.c_void_p, ctypes.c_void_p]),
    "chipe_open_ragged_dev": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_uint64, ctypes.c_void_p, c_u64p, c_u64p,
                                             ctypes.c_uint64, ctypes.c_void_p, c_u64p, c_u64p, ctypes.c_void_p,
                                             ctypes.c_void_p, ctypes.c_void_p]),
    "chipe_encode_scratch_len": (ctypes.c_uint64, [ctypes.c_uint8, c_u64p, ctypes.c_uint64]),
    "chipe_decode_scratch_len": (ctypes.c_uint64, [ctypes.c_uint8, c_u64p, ctypes.c_uint64]),
    "chipe_encode_ragged_dev": (ctypes.c_int, [ctypes.c_uint8, ctypes.c_void_p, ctypes.c_uint64,
                                               ctypes.POINTER(EciesInjectC), ctypes.c_void_p, c_u64p, c_u64p,
                                               ctypes.c_uint64, ctypes.c_void_p, c_u64p, c_u64p, ctypes.c_void_p,
                                               ctypes.POINTER(EncodeInfoC), ctypes.c_void_p, ctypes.c_void_p]),
    "chipe_decode_ragged_dev": (ctypes.c_int, [ctypes.c_uint8, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_void_p,
                                               c_u64p, c_u64p, ctypes.c_uint64, ctypes.c_void_p, c_u32p,
                                               ctypes.c_void_p, c_u64p, c_u64p, ctypes.c_void_p, ctypes.c_void_p,
                                               ctypes.c_void_p]),
}

# the snap header (include/carbonado_hip_snap.h): the snappy framing format over
# resident objects and the one-call forms of the levels with the Snappy bit, an
# eighth table of its own
SNAP_SIGNATURES = {
    "chips_abi_version": (ctypes.c_int, []),
    "chips_snap_scratch_len": (ctypes.c_uint64, [c_u64p, ctypes.c_uint64]),
    "chips_unsnap_scratch_len": (ctypes.c_uint64, [c_u64p, c_u64p, ctypes.c_uint64]),
    "chips_snap_ragged_dev": (ctypes.c_int, [ctypes.c_void_p, c_u64p, c_u64p, ctypes.c_uint64, ctypes.c_void_p,
                                             c_u64p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint64,
                                             ctypes.c_void_p]),
    "chips_unsnap_ragged_dev": (ctypes.c_int, [ctypes.c_void_p, c_u64p, c_u64p, ctypes.c_uint64, ctypes.c_void_p,
                                               c_u64p, c_u64p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
                                               ctypes.c_uint64, ctypes.c_void_p]),
    "chips_encode_layout": (ctypes.c_int, [ctypes.c_uint8, c_u64p, ctypes.c_uint64, ctypes.c_uint64, ctypes.c_uint64,
                                           c_u64p, c_u64p, c_u64p]),
    "chips_encode_scratch_len": (ctypes.c_uint64, [ctypes.c_uint8, c_u64p, ctypes.c_uint64]),
    "chips_decode_scratch_len": (ctypes.c_uint64, [ctypes.c_uint8, c_u64p, c_u64p, ctypes.c_uint64]),
    "chips_encode_ragged_dev": (ctypes.c_int, [ctypes.c_uint8, ctypes.c_void_p, ctypes.c_uint64,
                                               ctypes.POINTER(EciesInjectC), ctypes.c_void_p, c_u64p, c_u64p,
                                               ctypes.c_uint64, ctypes.c_void_p, c_u64p, c_u64p, ctypes.c_void_p,
                                               ctypes.POINTER(EncodeInfoC), ctypes.c_void_p, ctypes.c_void_p]),
    "chips_decode_ragged_dev": (ctypes.c_int, [ctypes.c_uint8, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_void_p,
                                               c_u64p, c_u64p, ctypes.c_uint64, ctypes.c_void_p, c_u32p,
                                               ctypes.c_void_p, c_u64p, c_u64p, ctypes.c_void_p, ctypes.c_void_p,
                                               ctypes.c_void_p, ctypes.c_void_p]),
}

# the cread header (include/carbonado_hip_cread.h): plaintext ranged reads of
# level-13 streams (the keystream over ranges, the keys of resident streams, the
# read), a ninth table of its own
CREAD_SIGNATURES = {
    "chipc_abi_version": (ctypes.c_int, []),
    "chipc_ctr_scratch_len": (ctypes.c_uint64, [ctypes.c_uint64, ctypes.c_uint64]),
    "chipc_ctr_ranges_dev": (ctypes.c_int, [c_u8p, c_u8p, ctypes.c_uint64, c_u32p, c_u64p, c_u64p, ctypes.c_uint64,
                                            ctypes.c_void_p, c_u64p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint64,
                                            ctypes.c_void_p]),
    "chipc_stream_keys_scratch_len": (ctypes.c_uint64, [ctypes.c_uint64]),
    "chipc_stream_keys_dev": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_uint64, ctypes.c_void_p, c_u64p, c_u64p,
                                             ctypes.c_void_p, c_u32p, c_u32p, ctypes.c_uint64, c_u8p, c_u8p, c_u32p,
                                             ctypes.c_void_p, ctypes.c_uint64, ctypes.c_void_p]),
    "chipc_read_layout": (ctypes.c_int, [c_u32p, c_u32p, ctypes.c_uint64, c_u32p, c_u64p, c_u64p, ctypes.c_uint64,
                                         ctypes.c_uint64, c_u64p, c_u64p, c_u64p, c_u64p]),
    "chipc_read_scratch_len": (ctypes.c_uint64, [ctypes.c_uint64, ctypes.c_uint64, ctypes.c_uint64]),
    "chipc_read_ranges_dev": (ctypes.c_int, [c_u8p, c_u8p, c_u32p, ctypes.c_void_p, c_u64p, c_u64p, ctypes.c_void_p,
                                             c_u32p, c_u32p, ctypes.c_uint64, c_u32p, c_u64p, c_u64p, ctypes.c_uint64,
                                             ctypes.c_void_p, c_u64p, c_u64p, ctypes.c_void_p, ctypes.c_void_p,
                                             ctypes.c_void_p, ctypes.c_uint32, ctypes.c_void_p, ctypes.c_uint64,
                                             ctypes.c_void_p]),
}

# the fread header (include/carbonado_hip_fread.h): plaintext ranged reads of
# level-14 and level-15 streams (the index check, the index build, the read),
# a tenth table of its own
FREAD_SIGNATURES = {
    "chipf_abi_version": (ctypes.c_int, []),
    "chipf_index_scratch_len": (ctypes.c_uint64, [ctypes.c_uint64, ctypes.c_uint64]),
    "chipf_verify_index_dev": (ctypes.c_int, [ctypes.c_uint8, c_u8p, c_u8p, c_u32p, ctypes.c_void_p, c_u64p, c_u64p,
                                              ctypes.c_void_p, c_u32p, c_u32p, ctypes.c_uint64, c_u64p, c_u64p, c_u64p,
                                              ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
                                              ctypes.c_uint64, ctypes.c_void_p]),
    "chipf_frame_index_dev": (ctypes.c_int, [ctypes.c_uint8, c_u8p, c_u8p, c_u32p, ctypes.c_void_p, c_u64p, c_u64p,
                                             ctypes.c_void_p, c_u32p, c_u32p, ctypes.c_uint64, c_u64p, c_u64p, c_u64p,
                                             c_u64p, c_u32p, c_u64p, c_u32p, ctypes.c_void_p, ctypes.c_uint64,
                                             ctypes.c_void_p]),
    "chipf_read_layout": (ctypes.c_int, [ctypes.c_uint8, c_u32p, c_u32p, c_u32p, c_u64p, c_u64p, c_u64p, c_u64p,
                                         ctypes.c_uint64, c_u32p, c_u64p, c_u64p, ctypes.c_uint64, ctypes.c_uint64,
                                         c_u64p, c_u64p, c_u64p, c_u64p, c_u64p, c_u64p]),
    "chipf_read_scratch_len": (ctypes.c_uint64, [ctypes.c_uint64, ctypes.c_uint64, ctypes.c_uint64, ctypes.c_uint64,
                                                 ctypes.c_uint64]),
    "chipf_read_ranges_dev": (ctypes.c_int, [ctypes.c_uint8, c_u8p, c_u8p, c_u32p, c_u64p, c_u64p, c_u64p, c_u64p,
                                             ctypes.c_void_p, c_u64p, c_u64p, ctypes.c_void_p, c_u32p, c_u32p,
                                             ctypes.c_uint64, c_u32p, c_u64p, c_u64p, ctypes.c_uint64, ctypes.c_void_p,
                                             c_u64p, c_u64p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
                                             ctypes.c_uint32, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_void_p]),
}

# the qread header (include/carbonado_hip_qread.h): ranged reads planned on the
# device from requests in device memory, an eleventh table of its own
class TableInfo(ctypes.Structure):
    """chipq_table_info: what the planned reads know of a stream table."""
    _fields_ = [("nstreams", ctypes.c_uint64), ("max_chunks", ctypes.c_uint64), ("min_shard", ctypes.c_uint64),
                ("reserved", ctypes.c_uint64)]


c_infop = ctypes.POINTER(TableInfo)
QREAD_SIGNATURES = {
    "chipq_abi_version": (ctypes.c_int, []),
    "chipq_stream_table_len": (ctypes.c_uint64, [ctypes.c_uint64]),
    "chipq_stream_table_dev": (ctypes.c_int, [ctypes.c_void_p, c_u64p, c_u64p, ctypes.c_void_p, c_u32p, c_u32p,
                                              ctypes.c_uint64, ctypes.c_void_p, ctypes.c_uint64, c_infop,
                                              ctypes.c_void_p]),
    "chipq_read_scratch_len": (ctypes.c_uint64, [c_infop, ctypes.c_uint64, ctypes.c_uint64, ctypes.c_uint32]),
    "chipq_read_ranges_dev": (ctypes.c_int, [ctypes.c_void_p, c_infop, ctypes.c_void_p, ctypes.c_void_p,
                                             ctypes.c_void_p, ctypes.c_uint64, ctypes.c_uint64, ctypes.c_void_p,
                                             ctypes.c_uint64, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
                                             ctypes.c_void_p, ctypes.c_uint64, ctypes.c_void_p]),
    "chipq_read_ranges_vouched_dev": (ctypes.c_int, [ctypes.c_void_p, c_infop, ctypes.c_void_p, ctypes.c_void_p,
                                                     ctypes.c_void_p, ctypes.c_uint64, ctypes.c_uint64,
                                                     ctypes.c_void_p, ctypes.c_uint64, ctypes.c_void_p,
                                                     ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
                                                     ctypes.c_uint32, ctypes.c_void_p, ctypes.c_uint64,
                                                     ctypes.c_void_p]),
}

# the kread header (include/carbonado_hip_kread.h): plaintext ranged reads of
# level-13 streams planned on the device over a resident key table, a twelfth
# table of its own
KREAD_SIGNATURES = {
    "chipk_abi_version": (ctypes.c_int, []),
    "chipk_key_table_len": (ctypes.c_uint64, [ctypes.c_uint64]),
    "chipk_key_table_dev": (ctypes.c_int, [c_u8p, c_u8p, c_u32p, ctypes.c_uint64, ctypes.c_void_p, ctypes.c_uint64,
                                           ctypes.c_void_p]),
    "chipk_key_table_wipe_dev": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_uint64, ctypes.c_void_p]),
    "chipk_read_scratch_len": (ctypes.c_uint64, [c_infop, ctypes.c_uint64, ctypes.c_uint64]),
    "chipk_read_ranges_dev": (ctypes.c_int, [ctypes.c_void_p, c_infop, ctypes.c_void_p, ctypes.c_uint64,
                                             ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint64,
                                             ctypes.c_uint64, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_void_p,
                                             ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint32,
                                             ctypes.c_void_p, ctypes.c_uint64, ctypes.c_void_p]),
}


# the gread header (include/carbonado_hip_gread.h): plaintext ranged reads of
# level-14 / level-15 streams planned on the device over a resident frame
# table, a thirteenth table of its own
class FrameInfo(ctypes.Structure):
    """chipg_frame_info: what the planned reads know of a frame table."""
    _fields_ = [("nstreams", ctypes.c_uint64), ("nentries", ctypes.c_uint64), ("max_frame", ctypes.c_uint64),
                ("format", ctypes.c_uint64)]


c_finfop = ctypes.POINTER(FrameInfo)
GREAD_SIGNATURES = {
    "chipg_abi_version": (ctypes.c_int, []),
    "chipg_frame_table_len": (ctypes.c_uint64, [ctypes.c_uint64, ctypes.c_uint64]),
    "chipg_frame_table_dev": (ctypes.c_int, [ctypes.c_uint8, c_u32p, c_u32p, c_u32p, c_u64p, c_u64p, c_u64p, c_u64p,
                                             ctypes.c_uint64, ctypes.c_void_p, ctypes.c_uint64, c_finfop,
                                             ctypes.c_void_p]),
    "chipg_read_scratch_len": (ctypes.c_uint64, [c_infop, c_finfop, ctypes.c_uint64, ctypes.c_uint64]),
    "chipg_read_ranges_dev": (ctypes.c_int, [ctypes.c_void_p, c_infop, ctypes.c_void_p, c_finfop, ctypes.c_void_p,
                                             ctypes.c_uint64, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
                                             ctypes.c_uint64, ctypes.c_uint64, ctypes.c_void_p, ctypes.c_uint64,
                                             ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
                                             ctypes.c_uint32, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_void_p]),
}


# the paudit header (include/carbonado_hip_paudit.h): slice audits planned on
# the device from requests (and proofs) in device memory, a fourteenth table of
# its own
class RootInfo(ctypes.Structure):
    """chipp_root_info: what the planned proof check knows of a root table."""
    _fields_ = [("nroots", ctypes.c_uint64), ("max_chunks", ctypes.c_uint64), ("reserved", ctypes.c_uint64 * 2)]


c_rinfop = ctypes.POINTER(RootInfo)
PAUDIT_SIGNATURES = {
    "chipp_abi_version": (ctypes.c_int, []),
    "chipp_root_table_len": (ctypes.c_uint64, [ctypes.c_uint64]),
    "chipp_root_table_dev": (ctypes.c_int, [c_u64p, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_void_p, ctypes.c_uint64,
                                            c_rinfop, ctypes.c_void_p]),
    "chipp_audit_scratch_len": (ctypes.c_uint64, [ctypes.c_uint64, ctypes.c_uint64, ctypes.c_uint64]),
    "chipp_proof_bound": (ctypes.c_uint64, [ctypes.c_uint64, ctypes.c_uint64]),
    "chipp_verify_slices_dev": (ctypes.c_int, [ctypes.c_void_p, c_infop, ctypes.c_void_p, ctypes.c_void_p,
                                               ctypes.c_void_p, ctypes.c_uint64, ctypes.c_uint64, ctypes.c_void_p,
                                               ctypes.c_uint64, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
                                               ctypes.c_uint64, ctypes.c_void_p]),
    "chipp_extract_slices_dev": (ctypes.c_int, [ctypes.c_void_p, c_infop, ctypes.c_void_p, ctypes.c_void_p,
                                                ctypes.c_void_p, ctypes.c_uint64, ctypes.c_uint64, ctypes.c_void_p,
                                                ctypes.c_uint64, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
                                                ctypes.c_uint64, ctypes.c_void_p]),
    "chipp_verify_proofs_dev": (ctypes.c_int, [ctypes.c_void_p, c_rinfop, ctypes.c_void_p, ctypes.c_void_p,
                                               ctypes.c_void_p, ctypes.c_uint64, ctypes.c_uint64, ctypes.c_void_p,
                                               ctypes.c_uint64, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint64,
                                               ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint64,
                                               ctypes.c_void_p]),
}

# the agree header (include/carbonado_hip_agree.h): the Ecies key agreement on
# the device and the envelope and one-call forms built on it, a fifteenth table
# of its own
AGREE_SIGNATURES = {
    "chipy_abi_version": (ctypes.c_int, []),
    "chipy_keys_scratch_len": (ctypes.c_uint64, [ctypes.c_uint64]),
    "chipy_seal_keys_dev": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_uint64, ctypes.c_void_p, ctypes.c_uint64,
                                           ctypes.c_void_p, ctypes.c_uint64, ctypes.c_void_p, ctypes.c_uint64,
                                           ctypes.c_void_p, ctypes.c_uint64, ctypes.c_void_p]),
    "chipy_open_keys_dev": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_uint64, ctypes.c_void_p, ctypes.c_uint64,
                                           ctypes.c_uint64, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_void_p,
                                           ctypes.c_void_p, ctypes.c_uint64, ctypes.c_void_p]),
    "chipy_envelope_scratch_len": (ctypes.c_uint64, [c_u64p, ctypes.c_uint64]),
    "chipy_seal_ragged_dev": ECIES_SIGNATURES["chipe_seal_ragged_dev"],
    "chipy_open_ragged_dev": ECIES_SIGNATURES["chipe_open_ragged_dev"],
    "chipy_encode_scratch_len": ECIES_SIGNATURES["chipe_encode_scratch_len"],
    "chipy_decode_scratch_len": ECIES_SIGNATURES["chipe_decode_scratch_len"],
    "chipy_encode_ragged_dev": ECIES_SIGNATURES["chipe_encode_ragged_dev"],
    "chipy_decode_ragged_dev": ECIES_SIGNATURES["chipe_decode_ragged_dev"],
    "chipy_key_table_scratch_len": (ctypes.c_uint64, [c_infop]),
    "chipy_key_table_dev": (ctypes.c_int, [ctypes.c_void_p, c_infop, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_void_p,
                                           ctypes.c_uint64, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_void_p]),
}

_LIB = None


def lib() -> ctypes.CDLL:
    """Load (once) and return the HIP library; raise if it is not built."""
    global _LIB
    if _LIB is None:
        if not LIB_PATH.exists():
            raise RuntimeError(
                f"{LIB_PATH} is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                "(there is no CPU fallback for the carbonado hot path)")
        # One HIP runtime per process.  torch's HIP libs NEED "libamdhip64.so"
        # (unversioned, RPATH $ORIGIN) while this library NEEDs the soname
        # "libamdhip64.so.7": loading torch first makes both bind to torch's
        # copy; the reverse order would map two runtimes.
        try:
            import torch  # noqa: F401
        except ImportError:  # torch is plumbing only; the library does not need it
            pass
        l = ctypes.CDLL(str(LIB_PATH))
        for name, (res, args) in {**SIGNATURES, **EXT_SIGNATURES, **AUDIT_SIGNATURES, **REPAIR_SIGNATURES,
                                  **READ_SIGNATURES, **VREAD_SIGNATURES, **ECIES_SIGNATURES,
                                  **SNAP_SIGNATURES, **CREAD_SIGNATURES, **FREAD_SIGNATURES,
                                  **QREAD_SIGNATURES, **KREAD_SIGNATURES, **GREAD_SIGNATURES,
                                  **PAUDIT_SIGNATURES, **AGREE_SIGNATURES}.items():
            fn = getattr(l, name)
            fn.restype = res
            fn.argtypes = args
        _LIB = l
    return _LIB
