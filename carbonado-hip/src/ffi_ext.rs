//! Raw declarations of `include/carbonado_hip_ext.h` (the `chipx_*` extension
//! entry points of `libcarbonado_hip.so`), kept apart from `ffi.rs`, which
//! mirrors the frozen drop-in header.  tests/test_ragged_cpu.py checks every
//! declaration against the header's prototype.
#![allow(non_camel_case_types)]

use std::os::raw::{c_int, c_void};

use crate::ffi::chip_encode_info;

pub const CHIPX_ABI_VERSION: c_int = 1;

extern "C" {
    pub fn chipx_abi_version() -> c_int;
    pub fn chipx_ragged_layout(format: u8, n: *const u64, count: u64, align: u64, stream_offset: u64,
                               out_off: *mut u64, out_len: *mut u64, total: *mut u64) -> c_int;
    pub fn chipx_ragged_scratch_len(format: u8, len: *const u64, count: u64, decode: c_int) -> u64;
    pub fn chipx_encode_ragged_dev(format: u8, d_in: *const u8, in_off: *const u64, n: *const u64, count: u64,
                                   d_out: *mut u8, out_off: *const u64, out_len: *mut u64, d_hash: *mut u8,
                                   info: *mut chip_encode_info, d_scratch: *mut c_void, stream: *mut c_void) -> c_int;
    pub fn chipx_decode_ragged_dev(format: u8, d_in: *const u8, in_off: *const u64, in_len: *const u64, count: u64,
                                   d_hash: *const u8, padding: *const u32, d_out: *mut u8, out_off: *const u64,
                                   out_len: *mut u64, d_status: *mut u32, d_scratch: *mut c_void,
                                   stream: *mut c_void) -> c_int;
}
