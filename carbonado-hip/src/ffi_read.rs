//! Raw declarations of `include/carbonado_hip_read.h` (the `chipd_*` ranged
//! reads of `libcarbonado_hip.so`), kept apart from `ffi.rs`, `ffi_ext.rs`,
//! `ffi_audit.rs` and `ffi_repair.rs`, whose headers stay frozen.
//! tests/test_read_cpu.py checks every declaration against the header's
//! prototype.
#![allow(non_camel_case_types)]

use std::os::raw::{c_int, c_void};

pub const CHIPD_ABI_VERSION: c_int = 1;

extern "C" {
    pub fn chipd_abi_version() -> c_int;
    pub fn chipd_read_layout(chunk_len: *const u32, padding: *const u32, nstreams: u64, req_stream: *const u32,
                             start: *const u64, len: *const u64, nreq: u64, align: u64, content_off: *mut u64,
                             content_len: *mut u64, content_total: *mut u64, nseg: *mut u64) -> c_int;
    pub fn chipd_read_scratch_len(nreq: u64, nseg: u64) -> u64;
    pub fn chipd_read_ranges_dev(d_streams: *const u8, in_off: *const u64, in_len: *const u64, d_hash: *const u8,
                                 padding: *const u32, chunk_len: *const u32, nstreams: u64, req_stream: *const u32,
                                 start: *const u64, len: *const u64, nreq: u64, d_content: *mut u8,
                                 content_off: *const u64, content_len: *mut u64, d_status: *mut u32,
                                 d_used: *mut u32, d_scratch: *mut c_void, scratch_len: u64, stream: *mut c_void)
                                 -> c_int;
}
