//! Raw declarations of `include/carbonado_hip_gread.h` (the `chipg_*` plaintext
//! ranged reads of level-14 and level-15 objects planned on the device of
//! `libcarbonado_hip.so`), kept apart from the twelve older `ffi*.rs` files,
//! whose headers stay frozen.
//! tests/test_gread_cpu.py checks every declaration against the header's
//! prototype.
use std::os::raw::{c_int, c_void};

use crate::ffi_qread::chipq_table_info;

pub const CHIPG_ABI_VERSION: c_int = 1;

/// What the read calls know of a frame table (host memory).
#[repr(C)]
#[derive(Debug, Clone, Copy, Default, PartialEq, Eq)]
pub struct chipg_frame_info {
    pub nstreams: u64,
    pub nentries: u64,
    pub max_frame: u64,
    pub format: u64,
}

extern "C" {
    pub fn chipg_abi_version() -> c_int;
    pub fn chipg_frame_table_len(nstreams: u64, nentries: u64) -> u64;
    pub fn chipg_frame_table_dev(format: u8, chunk_len: *const u32, padding: *const u32, index_status: *const u32,
                                 frame_off: *const u64, idx_off: *const u64, nframes: *const u64,
                                 plain_len: *const u64, nstreams: u64, d_ftable: *mut c_void, ftable_len: u64,
                                 finfo: *mut chipg_frame_info, stream: *mut c_void)
                                 -> c_int;
    pub fn chipg_read_scratch_len(info: *const chipq_table_info, finfo: *const chipg_frame_info, nreq: u64,
                                  max_len: u64) -> u64;
    pub fn chipg_read_ranges_dev(d_table: *const c_void, info: *const chipq_table_info, d_ftable: *const c_void,
                                 finfo: *const chipg_frame_info, d_keytab: *const c_void, keytab_len: u64,
                                 d_req_stream: *const u32, d_start: *const u64, d_len: *const u64, nreq: u64,
                                 max_len: u64, d_content: *mut u8, content_stride: u64, d_content_len: *mut u64,
                                 d_status: *mut u32, d_used: *mut u32, d_vouch: *mut u32, flags: u32,
                                 d_scratch: *mut c_void, scratch_len: u64, stream: *mut c_void)
                                 -> c_int;
}
