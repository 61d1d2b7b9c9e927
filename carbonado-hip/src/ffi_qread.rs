//! Raw declarations of `include/carbonado_hip_qread.h` (the `chipq_*` ranged
//! reads planned on the device of `libcarbonado_hip.so`), kept apart from the
//! ten older `ffi*.rs` files, whose headers stay frozen.
//! tests/test_qread_cpu.py checks every declaration against the header's
//! prototype.
#![allow(non_camel_case_types)]

use std::os::raw::{c_int, c_void};

pub const CHIPQ_ABI_VERSION: c_int = 1;

/// What the read calls know of a stream table (host memory).
#[repr(C)]
#[derive(Debug, Clone, Copy, Default, PartialEq, Eq)]
pub struct chipq_table_info {
    pub nstreams: u64,
    pub max_chunks: u64,
    pub min_shard: u64,
    pub reserved: u64,
}

extern "C" {
    pub fn chipq_abi_version() -> c_int;
    pub fn chipq_stream_table_len(nstreams: u64) -> u64;
    pub fn chipq_stream_table_dev(d_streams: *const u8, in_off: *const u64, in_len: *const u64, d_hash: *const u8,
                                  padding: *const u32, chunk_len: *const u32, nstreams: u64, d_table: *mut c_void,
                                  table_len: u64, info: *mut chipq_table_info, stream: *mut c_void)
                                  -> c_int;
    pub fn chipq_read_scratch_len(info: *const chipq_table_info, nreq: u64, max_len: u64, vouched: u32) -> u64;
    pub fn chipq_read_ranges_dev(d_table: *const c_void, info: *const chipq_table_info, d_req_stream: *const u32,
                                 d_start: *const u64, d_len: *const u64, nreq: u64, max_len: u64, d_content: *mut u8,
                                 content_stride: u64, d_content_len: *mut u64, d_status: *mut u32, d_used: *mut u32,
                                 d_scratch: *mut c_void, scratch_len: u64, stream: *mut c_void)
                                 -> c_int;
    pub fn chipq_read_ranges_vouched_dev(d_table: *const c_void, info: *const chipq_table_info,
                                         d_req_stream: *const u32, d_start: *const u64, d_len: *const u64, nreq: u64,
                                         max_len: u64, d_content: *mut u8, content_stride: u64,
                                         d_content_len: *mut u64, d_status: *mut u32, d_used: *mut u32,
                                         d_vouch: *mut u32, flags: u32, d_scratch: *mut c_void, scratch_len: u64,
                                         stream: *mut c_void)
                                         -> c_int;
}
