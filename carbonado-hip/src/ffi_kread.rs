//! Raw declarations of `include/carbonado_hip_kread.h` (the `chipk_*` plaintext
//! ranged reads of level-13 objects planned on the device of
//! `libcarbonado_hip.so`), kept apart from the eleven older `ffi*.rs` files,
//! whose headers stay frozen.
//! tests/test_kread_cpu.py checks every declaration against the header's
//! prototype.
use std::os::raw::{c_int, c_void};

use crate::ffi_qread::chipq_table_info;

pub const CHIPK_ABI_VERSION: c_int = 1;

extern "C" {
    pub fn chipk_abi_version() -> c_int;
    pub fn chipk_key_table_len(nstreams: u64) -> u64;
    pub fn chipk_key_table_dev(keys: *const u8, ivs: *const u8, key_status: *const u32, nstreams: u64,
                               d_keytab: *mut c_void, keytab_len: u64, stream: *mut c_void)
                               -> c_int;
    pub fn chipk_key_table_wipe_dev(d_keytab: *mut c_void, keytab_len: u64, stream: *mut c_void) -> c_int;
    pub fn chipk_read_scratch_len(info: *const chipq_table_info, nreq: u64, max_len: u64) -> u64;
    pub fn chipk_read_ranges_dev(d_table: *const c_void, info: *const chipq_table_info, d_keytab: *const c_void,
                                 keytab_len: u64, d_req_stream: *const u32, d_start: *const u64, d_len: *const u64,
                                 nreq: u64, max_len: u64, d_content: *mut u8, content_stride: u64,
                                 d_content_len: *mut u64, d_status: *mut u32, d_used: *mut u32, d_vouch: *mut u32,
                                 flags: u32, d_scratch: *mut c_void, scratch_len: u64, stream: *mut c_void)
                                 -> c_int;
}
