//! Raw declarations of `include/carbonado_hip_snap.h` (the `chips_*` snappy
//! calls over device-resident objects of `libcarbonado_hip.so`), kept apart
//! from `ffi.rs`, `ffi_ext.rs`, `ffi_audit.rs`, `ffi_repair.rs`, `ffi_read.rs`,
//! `ffi_vread.rs` and `ffi_ecies.rs`, whose headers stay frozen.
//! tests/test_snap_dev_cpu.py checks every declaration against the header's
//! prototype.
#![allow(non_camel_case_types)]

use std::os::raw::{c_int, c_void};

use crate::ffi::{chip_ecies_inject, chip_encode_info};

pub const CHIPS_ABI_VERSION: c_int = 1;

extern "C" {
    pub fn chips_abi_version() -> c_int;
    pub fn chips_snap_scratch_len(n: *const u64, count: u64) -> u64;
    pub fn chips_unsnap_scratch_len(in_len: *const u64, out_cap: *const u64, count: u64) -> u64;
    pub fn chips_snap_ragged_dev(d_in: *const u8, in_off: *const u64, n: *const u64, count: u64, d_out: *mut u8,
                                 out_off: *const u64, d_out_len: *mut u64, d_scratch: *mut c_void, scratch_len: u64,
                                 stream: *mut c_void)
                                 -> c_int;
    pub fn chips_unsnap_ragged_dev(d_in: *const u8, in_off: *const u64, in_len: *const u64, count: u64,
                                   d_out: *mut u8, out_off: *const u64, out_cap: *const u64, d_out_len: *mut u64,
                                   d_status: *mut u32, d_scratch: *mut c_void, scratch_len: u64, stream: *mut c_void)
                                   -> c_int;
    pub fn chips_encode_layout(format: u8, n: *const u64, count: u64, align: u64, stream_offset: u64,
                               out_off: *mut u64, out_cap: *mut u64, total: *mut u64)
                               -> c_int;
    pub fn chips_encode_scratch_len(format: u8, n: *const u64, count: u64) -> u64;
    pub fn chips_decode_scratch_len(format: u8, in_len: *const u64, out_cap: *const u64, count: u64) -> u64;
    pub fn chips_encode_ragged_dev(format: u8, pubkey: *const u8, pubkey_len: u64, inject: *const chip_ecies_inject,
                                   d_in: *const u8, in_off: *const u64, n: *const u64, count: u64, d_out: *mut u8,
                                   out_off: *const u64, out_len: *mut u64, d_hash: *mut u8,
                                   info: *mut chip_encode_info, d_scratch: *mut c_void, stream: *mut c_void)
                                   -> c_int;
    pub fn chips_decode_ragged_dev(format: u8, secret_key: *const u8, sk_len: u64, d_in: *const u8,
                                   in_off: *const u64, in_len: *const u64, count: u64, d_hash: *const u8,
                                   padding: *const u32, d_out: *mut u8, out_off: *const u64, out_cap: *const u64,
                                   d_out_len: *mut u64, d_status: *mut u32, d_scratch: *mut c_void,
                                   stream: *mut c_void)
                                   -> c_int;
}
