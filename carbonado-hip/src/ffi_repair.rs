//! Raw declarations of `include/carbonado_hip_repair.h` (the `chipr_*` ragged
//! scrub of `libcarbonado_hip.so`), kept apart from `ffi.rs`, `ffi_ext.rs` and
//! `ffi_audit.rs`, whose headers stay frozen.  tests/test_repair_cpu.py checks
//! every declaration against the header's prototype.
#![allow(non_camel_case_types)]

use std::os::raw::{c_int, c_void};

pub const CHIPR_ABI_VERSION: c_int = 1;

extern "C" {
    pub fn chipr_abi_version() -> c_int;
    pub fn chipr_scrub_ragged_scratch_len(in_len: *const u64, count: u64, nrepair: u64) -> u64;
    pub fn chipr_shard_masks_ragged_dev(d_in: *const u8, in_off: *const u64, in_len: *const u64, count: u64,
                                        d_hash: *const u8, chunk_len: *const u32, d_masks: *mut u32,
                                        d_scratch: *mut c_void, scratch_len: u64, stream: *mut c_void) -> c_int;
    pub fn chipr_scrub_ragged_dev(d_in: *const u8, in_off: *const u64, in_len: *const u64, count: u64,
                                  d_hash: *const u8, padding: *const u32, chunk_len: *const u32, d_out: *mut u8,
                                  out_off: *const u64, status: *mut i32, d_scratch: *mut c_void, scratch_len: u64,
                                  stream: *mut c_void) -> c_int;
}
