//! Raw declarations of `include/carbonado_hip_audit.h` (the `chipa_*` slice
//! audits of `libcarbonado_hip.so`), kept apart from `ffi.rs` and
//! `ffi_ext.rs`, whose headers stay frozen.  tests/test_audit_cpu.py checks
//! every declaration against the header's prototype.
#![allow(non_camel_case_types)]

use std::os::raw::{c_int, c_void};

pub const CHIPA_ABI_VERSION: c_int = 1;

extern "C" {
    pub fn chipa_abi_version() -> c_int;
    pub fn chipa_slice_layout(content_len: *const u64, index: *const u64, count: *const u64, nreq: u64, align: u64,
                              proof_off: *mut u64, proof_len: *mut u64, content_off: *mut u64,
                              content_len_out: *mut u64, proof_total: *mut u64, content_total: *mut u64) -> c_int;
    pub fn chipa_audit_scratch_len(nstreams: u64, nreq: u64) -> u64;
    pub fn chipa_extract_slices_dev(d_streams: *const u8, in_off: *const u64, in_len: *const u64, nstreams: u64,
                                    req_stream: *const u32, index: *const u64, count: *const u64, nreq: u64,
                                    d_proofs: *mut u8, proof_off: *const u64, proof_len: *const u64,
                                    d_scratch: *mut c_void, stream: *mut c_void) -> c_int;
    pub fn chipa_verify_slices_dev(d_streams: *const u8, in_off: *const u64, in_len: *const u64, d_hash: *const u8,
                                   nstreams: u64, req_stream: *const u32, index: *const u64, count: *const u64,
                                   nreq: u64, d_content: *mut u8, content_off: *const u64, content_len: *mut u64,
                                   d_status: *mut u32, d_scratch: *mut c_void, stream: *mut c_void) -> c_int;
    pub fn chipa_verify_proofs_dev(d_proofs: *const u8, proof_off: *const u64, proof_len: *const u64,
                                   content_len: *const u64, d_hash: *const u8, index: *const u64, count: *const u64,
                                   nreq: u64, d_content: *mut u8, content_off: *const u64,
                                   content_len_out: *mut u64, d_status: *mut u32, d_scratch: *mut c_void,
                                   stream: *mut c_void) -> c_int;
}
