//! Raw declarations of `include/carbonado_hip_fread.h` (the `chipf_*` plaintext
//! ranged reads of level-14 and level-15 streams in `libcarbonado_hip.so`),
//! kept apart from the nine older `ffi*.rs` files, whose headers stay frozen.
//! tests/test_fread_cpu.py checks every declaration against the header's
//! prototype.
#![allow(non_camel_case_types)]

use std::os::raw::{c_int, c_void};

pub const CHIPF_ABI_VERSION: c_int = 1;

extern "C" {
    pub fn chipf_abi_version() -> c_int;
    pub fn chipf_index_scratch_len(nstreams: u64, nentries: u64) -> u64;
    pub fn chipf_verify_index_dev(format: u8, keys: *const u8, ivs: *const u8, key_status: *const u32,
                                  d_streams: *const u8, in_off: *const u64, in_len: *const u64, d_hash: *const u8,
                                  padding: *const u32, chunk_len: *const u32, nstreams: u64, frame_off: *const u64,
                                  idx_off: *const u64, nframes: *const u64, d_index_status: *mut u32,
                                  d_plain_len: *mut u64, d_index_vouch: *mut u32, d_scratch: *mut c_void,
                                  scratch_len: u64, stream: *mut c_void)
                                  -> c_int;
    pub fn chipf_frame_index_dev(format: u8, keys: *const u8, ivs: *const u8, key_status: *const u32,
                                 d_streams: *const u8, in_off: *const u64, in_len: *const u64, d_hash: *const u8,
                                 padding: *const u32, chunk_len: *const u32, nstreams: u64, frame_off: *mut u64,
                                 idx_off: *const u64, idx_cap: *const u64, nframes: *mut u64, index_status: *mut u32,
                                 plain_len: *mut u64, index_vouch: *mut u32, d_scratch: *mut c_void, scratch_len: u64,
                                 stream: *mut c_void)
                                 -> c_int;
    pub fn chipf_read_layout(format: u8, chunk_len: *const u32, padding: *const u32, index_status: *const u32,
                             frame_off: *const u64, idx_off: *const u64, nframes: *const u64,
                             plain_len: *const u64, nstreams: u64,
                             req_stream: *const u32, start: *const u64, len: *const u64, nreq: u64, align: u64,
                             content_off: *mut u64, content_len: *mut u64, content_total: *mut u64, nseg: *mut u64,
                             stage_total: *mut u64, vseg: *mut u64)
                             -> c_int;
    pub fn chipf_read_scratch_len(nreq: u64, nseg: u64, stage_total: u64, vseg: u64, nstreams: u64) -> u64;
    pub fn chipf_read_ranges_dev(format: u8, keys: *const u8, ivs: *const u8, index_status: *const u32,
                                 frame_off: *const u64, idx_off: *const u64, nframes: *const u64,
                                 plain_len: *const u64, d_streams: *const u8, in_off: *const u64, in_len: *const u64,
                                 d_hash: *const u8, padding: *const u32, chunk_len: *const u32, nstreams: u64,
                                 req_stream: *const u32, start: *const u64, len: *const u64, nreq: u64,
                                 d_content: *mut u8, content_off: *const u64, content_len: *mut u64,
                                 d_status: *mut u32, d_used: *mut u32, d_vouch: *mut u32, flags: u32,
                                 d_scratch: *mut c_void, scratch_len: u64, stream: *mut c_void)
                                 -> c_int;
}
