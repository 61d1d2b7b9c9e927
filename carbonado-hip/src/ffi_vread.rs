//! Raw declarations of `include/carbonado_hip_vread.h` (the `chipv_*` vouched
//! ranged reads of `libcarbonado_hip.so`), kept apart from `ffi.rs`,
//! `ffi_ext.rs`, `ffi_audit.rs`, `ffi_repair.rs` and `ffi_read.rs`, whose
//! headers stay frozen.  tests/test_vread_cpu.py checks every declaration
//! against the header's prototype.
#![allow(non_camel_case_types)]

use std::os::raw::{c_int, c_void};

pub const CHIPV_ABI_VERSION: c_int = 1;

/// bits of a request's vouch word
pub const CHIPV_VOUCHED: u32 = 1;
pub const CHIPV_UNVOUCHED: u32 = 2;
pub const CHIPV_CONTRADICTED: u32 = 4;

/// flag: a request with an unvouched segment fails
pub const CHIPV_STRICT: u32 = 1;

extern "C" {
    pub fn chipv_abi_version() -> c_int;
    pub fn chipv_read_scratch_len(nreq: u64, nseg: u64) -> u64;
    pub fn chipv_read_ranges_dev(d_streams: *const u8, in_off: *const u64, in_len: *const u64, d_hash: *const u8,
                                 padding: *const u32, chunk_len: *const u32, nstreams: u64, req_stream: *const u32,
                                 start: *const u64, len: *const u64, nreq: u64, d_content: *mut u8,
                                 content_off: *const u64, content_len: *mut u64, d_status: *mut u32,
                                 d_used: *mut u32, d_vouch: *mut u32, flags: u32, d_scratch: *mut c_void,
                                 scratch_len: u64, stream: *mut c_void)
                                 -> c_int;
}
