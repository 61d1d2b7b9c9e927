//! Raw declarations of `include/carbonado_hip_agree.h` (the `chipy_*` calls of
//! `libcarbonado_hip.so`: the Ecies key agreement on the device and the
//! envelope and one-call forms built on it), kept apart from the fourteen older
//! `ffi*.rs` files, whose headers stay frozen.  tests/test_agree_cpu.py checks
//! every declaration against the header's prototype.
#![allow(non_camel_case_types)]

use std::os::raw::{c_int, c_void};

use crate::ffi::{chip_ecies_inject, chip_encode_info};
use crate::ffi_qread::chipq_table_info;

pub const CHIPY_ABI_VERSION: c_int = 1;

extern "C" {
    pub fn chipy_abi_version() -> c_int;
    pub fn chipy_keys_scratch_len(count: u64) -> u64;
    pub fn chipy_seal_keys_dev(pubkey: *const u8, pubkey_len: u64, eph_sk: *const u8, count: u64, d_pub: *mut u8,
                               pub_pitch: u64, d_keys: *mut u8, key_pitch: u64, d_scratch: *mut c_void,
                               scratch_len: u64, stream: *mut c_void)
                               -> c_int;
    pub fn chipy_open_keys_dev(secret_key: *const u8, sk_len: u64, d_eph: *const u8, eph_pitch: u64, count: u64,
                               d_keys: *mut u8, key_pitch: u64, d_status: *mut u32, d_scratch: *mut c_void,
                               scratch_len: u64, stream: *mut c_void)
                               -> c_int;
    pub fn chipy_envelope_scratch_len(n: *const u64, count: u64) -> u64;
    pub fn chipy_seal_ragged_dev(pubkey: *const u8, pubkey_len: u64, inject: *const chip_ecies_inject,
                                 d_in: *const u8, in_off: *const u64, n: *const u64, count: u64, d_out: *mut u8,
                                 out_off: *const u64, d_scratch: *mut c_void, stream: *mut c_void)
                                 -> c_int;
    pub fn chipy_open_ragged_dev(secret_key: *const u8, sk_len: u64, d_in: *const u8, in_off: *const u64,
                                 in_len: *const u64, count: u64, d_out: *mut u8, out_off: *const u64,
                                 out_len: *mut u64, d_status: *mut u32, d_scratch: *mut c_void, stream: *mut c_void)
                                 -> c_int;
    pub fn chipy_encode_scratch_len(format: u8, n: *const u64, count: u64) -> u64;
    pub fn chipy_decode_scratch_len(format: u8, in_len: *const u64, count: u64) -> u64;
    pub fn chipy_encode_ragged_dev(format: u8, pubkey: *const u8, pubkey_len: u64, inject: *const chip_ecies_inject,
                                   d_in: *const u8, in_off: *const u64, n: *const u64, count: u64, d_out: *mut u8,
                                   out_off: *const u64, out_len: *mut u64, d_hash: *mut u8,
                                   info: *mut chip_encode_info, d_scratch: *mut c_void, stream: *mut c_void)
                                   -> c_int;
    pub fn chipy_decode_ragged_dev(format: u8, secret_key: *const u8, sk_len: u64, d_in: *const u8,
                                   in_off: *const u64, in_len: *const u64, count: u64, d_hash: *const u8,
                                   padding: *const u32, d_out: *mut u8, out_off: *const u64, out_len: *mut u64,
                                   d_status: *mut u32, d_scratch: *mut c_void, stream: *mut c_void)
                                   -> c_int;
    pub fn chipy_key_table_scratch_len(info: *const chipq_table_info) -> u64;
    pub fn chipy_key_table_dev(d_table: *const c_void, info: *const chipq_table_info, secret_key: *const u8,
                               sk_len: u64, d_keytab: *mut c_void, keytab_len: u64, d_scratch: *mut c_void,
                               scratch_len: u64, stream: *mut c_void)
                               -> c_int;
}
