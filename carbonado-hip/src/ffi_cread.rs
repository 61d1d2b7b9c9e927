//! Raw declarations of `include/carbonado_hip_cread.h` (the `chipc_*` plaintext
//! ranged reads of level-13 streams in `libcarbonado_hip.so`), kept apart from
//! the eight older `ffi*.rs` files, whose headers stay frozen.
//! tests/test_cread_cpu.py checks every declaration against the header's
//! prototype.
#![allow(non_camel_case_types)]

use std::os::raw::{c_int, c_void};

pub const CHIPC_ABI_VERSION: c_int = 1;

extern "C" {
    pub fn chipc_abi_version() -> c_int;
    pub fn chipc_ctr_scratch_len(nkeys: u64, nitems: u64) -> u64;
    pub fn chipc_ctr_ranges_dev(keys: *const u8, ivs: *const u8, nkeys: u64, item_key: *const u32, pos: *const u64,
                                n: *const u64, nitems: u64, d_buf: *mut u8, buf_off: *const u64, d_gate: *const u32,
                                d_scratch: *mut c_void, scratch_len: u64, stream: *mut c_void)
                                -> c_int;
    pub fn chipc_stream_keys_scratch_len(nstreams: u64) -> u64;
    pub fn chipc_stream_keys_dev(secret_key: *const u8, sk_len: u64, d_streams: *const u8, in_off: *const u64,
                                 in_len: *const u64, d_hash: *const u8, padding: *const u32, chunk_len: *const u32,
                                 nstreams: u64, keys_out: *mut u8, ivs_out: *mut u8, key_status: *mut u32,
                                 d_scratch: *mut c_void, scratch_len: u64, stream: *mut c_void)
                                 -> c_int;
    pub fn chipc_read_layout(chunk_len: *const u32, padding: *const u32, nstreams: u64, req_stream: *const u32,
                             start: *const u64, len: *const u64, nreq: u64, align: u64, content_off: *mut u64,
                             content_len: *mut u64, content_total: *mut u64, nseg: *mut u64)
                             -> c_int;
    pub fn chipc_read_scratch_len(nreq: u64, nseg: u64, nstreams: u64) -> u64;
    pub fn chipc_read_ranges_dev(keys: *const u8, ivs: *const u8, key_status: *const u32, d_streams: *const u8,
                                 in_off: *const u64, in_len: *const u64, d_hash: *const u8, padding: *const u32,
                                 chunk_len: *const u32, nstreams: u64, req_stream: *const u32, start: *const u64,
                                 len: *const u64, nreq: u64, d_content: *mut u8, content_off: *const u64,
                                 content_len: *mut u64, d_status: *mut u32, d_used: *mut u32, d_vouch: *mut u32,
                                 flags: u32, d_scratch: *mut c_void, scratch_len: u64, stream: *mut c_void)
                                 -> c_int;
}
