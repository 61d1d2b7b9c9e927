//! Raw declarations of `include/carbonado_hip_paudit.h` (the `chipp_*` slice
//! audits planned on the device of `libcarbonado_hip.so`), kept apart from the
//! thirteen older `ffi*.rs` files, whose headers stay frozen.
//! tests/test_paudit_cpu.py checks every declaration against the header's
//! prototype.
#![allow(non_camel_case_types)]

use std::os::raw::{c_int, c_void};

use crate::ffi_qread::chipq_table_info;

pub const CHIPP_ABI_VERSION: c_int = 1;

/// `d_req_stream[r]` of a spare slot.
pub const CHIPP_NO_REQUEST: u32 = 0xFFFF_FFFF;

/// What the planned proof check knows of a root table (host memory).
#[repr(C)]
#[derive(Debug, Clone, Copy, Default, PartialEq, Eq)]
pub struct chipp_root_info {
    pub nroots: u64,
    pub max_chunks: u64,
    pub reserved: [u64; 2],
}

extern "C" {
    pub fn chipp_abi_version() -> c_int;
    pub fn chipp_root_table_len(nroots: u64) -> u64;
    pub fn chipp_root_table_dev(content_len: *const u64, d_hash: *const u8, nroots: u64, d_table: *mut c_void,
                                table_len: u64, info: *mut chipp_root_info, stream: *mut c_void)
                                -> c_int;
    pub fn chipp_audit_scratch_len(info_max_chunks: u64, nreq: u64, max_count: u64) -> u64;
    pub fn chipp_proof_bound(max_chunks: u64, max_count: u64) -> u64;
    pub fn chipp_verify_slices_dev(d_table: *const c_void, info: *const chipq_table_info, d_req_stream: *const u32,
                                   d_index: *const u64, d_count: *const u64, nreq: u64, max_count: u64,
                                   d_content: *mut u8, content_stride: u64, d_content_len: *mut u64,
                                   d_status: *mut u32, d_scratch: *mut c_void, scratch_len: u64, stream: *mut c_void)
                                   -> c_int;
    pub fn chipp_extract_slices_dev(d_table: *const c_void, info: *const chipq_table_info, d_req_stream: *const u32,
                                    d_index: *const u64, d_count: *const u64, nreq: u64, max_count: u64,
                                    d_proofs: *mut u8, proof_stride: u64, d_proof_len: *mut u64, d_status: *mut u32,
                                    d_scratch: *mut c_void, scratch_len: u64, stream: *mut c_void)
                                    -> c_int;
    pub fn chipp_verify_proofs_dev(d_roots: *const c_void, root_info: *const chipp_root_info,
                                   d_req_stream: *const u32, d_index: *const u64, d_count: *const u64, nreq: u64,
                                   max_count: u64, d_proofs: *const u8, proof_stride: u64, d_proof_len: *const u64,
                                   d_content: *mut u8, content_stride: u64, d_content_len: *mut u64,
                                   d_status: *mut u32, d_scratch: *mut c_void, scratch_len: u64, stream: *mut c_void)
                                   -> c_int;
}
