//! carbonado-hip: the MI355X (gfx950) hot path of carbonado's encode()/decode()
//! behind safe Rust wrappers over `libcarbonado_hip.so` (`include/carbonado_hip.h`).
//!
//! * Stage functions, one per crate-internal seam of carbonado 0.6.0
//!   (SURVEY.md §8b): [`zfec_encode`] <- `encoding::zfec` (encoding.rs:48),
//!   [`bao_encode`] <- `encoding::bao` (encoding.rs:39), [`zfec_decode`] <-
//!   `decoding::zfec` (decoding.rs:35), [`zfec_decode_shares`] <-
//!   `decoding::zfec_chunks` (decoding.rs:21), [`bao_decode`] <- `decoding::bao`
//!   (decoding.rs:54).  Inputs are borrowed slices, outputs fresh `Vec<u8>`s, as
//!   in the crate; the library copies pageable memory through its own pinned
//!   ring, so nothing needs registering.
//! * The glue ([`encode`], [`decode`]), slices and scrub, the host stages,
//!   the flat-file header and the streaming [`BaoHasher`].
//! * The device-resident batch API (the throughput path the benchmark is
//!   measured on): [`DeviceRows`] allocates through `chip_device_alloc`, the
//!   library's class-balanced HBM allocator (the 4-of-8 encode
//!   runs at 0.77 of the HBM roofline over it, 0.64 over a plain hipMalloc),
//!   so Rust callers get the fast placement by default; caller-owned device
//!   memory can be wrapped with [`DeviceRows::from_raw`].
//!
//! There is no CPU fallback: with no gfx950 device every compute call returns
//! [`ChipError::NoDevice`].
pub mod ffi;
mod ffi_ext;
mod ffi_audit;
mod ffi_repair;
mod ffi_read;
mod ffi_vread;
mod ffi_ecies;
mod ffi_snap;
mod ffi_cread;
mod ffi_fread;
mod ffi_qread;
mod ffi_kread;
mod ffi_gread;
mod ffi_paudit;
mod ffi_agree;

use std::ffi::CStr;
use std::os::raw::{c_int, c_void};
use std::ptr;
use std::sync::OnceLock;

pub use ffi::chip_encode_info as ChipEncodeInfo;
pub use ffi::chip_header as ChipHeader;

pub const HASH_LEN: usize = ffi::CHIP_HASH_LEN;

/// One variant per `chip_status` (include/carbonado_hip.h), named after the
/// `CarbonadoError` variant it stands for (error.rs:7-115).
#[derive(Debug, Clone, PartialEq, Eq, thiserror::Error)]
pub enum ChipError {
    #[error("invalid argument")]
    InvalidArgument,
    #[error("output buffer too small: {0} bytes needed")]
    BufferTooSmall(u64),
    #[error("Input bytes must divide evenly over number of zfec chunks.")]
    UnevenZfecChunks,
    #[error("Hash must be 32 bytes long, an input of {0} bytes was provided.")]
    HashDecode(usize),
    #[error("bao decode: hash mismatch")]
    BaoHashMismatch,
    #[error("bao decode: truncated stream")]
    BaoTruncated,
    #[error("zfec: fewer than k distinct shares")]
    Zfec,
    #[error("Padding from Zfec should always be zero, since Carbonado adds its own padding.")]
    EncodeZfecPadding,
    #[error("Chunk length should be as calculated.")]
    EncodeInvalidChunkLength,
    #[error("Verifiable slice count should be evenly divisible by 8.")]
    InvalidVerifiableSliceCount,
    #[error("unsupported format bits")]
    UnsupportedFormat,
    #[error("Data does not need to be scrubbed.")]
    UnnecessaryScrub,
    #[error("Scrubbed padding should remain the same.")]
    ScrubbedPaddingMismatch,
    #[error("Mismatch between scrubbed data length and input length.")]
    ScrubbedLengthMismatch,
    #[error("Scrubbed hash is not equal to original hash.")]
    InvalidScrubbedHash,
    #[error("snappy framing error")]
    Snap,
    #[error("ecies error (bad key or tag)")]
    Ecies,
    #[error("secp256k1 error")]
    Secp256k1,
    #[error("Invalid header length calculation")]
    InvalidHeaderLength,
    #[error("File header lacks Carbonado magic number.")]
    InvalidMagic,
    #[error("no usable gfx950 device: {0}")]
    NoDevice(String),
    #[error("HIP runtime error: {0}")]
    Device(String),
    #[error("libcarbonado_hip has ABI {0}, this crate binds ABI {abi}", abi = ffi::CHIP_ABI_VERSION)]
    AbiMismatch(i32),
    #[error("status {0}: {1}")]
    Other(i32, String),
}

fn cstr(p: *const std::os::raw::c_char) -> String {
    if p.is_null() {
        return String::new();
    }
    unsafe { CStr::from_ptr(p) }.to_string_lossy().into_owned()
}

impl ChipError {
    /// The error for a non-zero status.  `hash_len` fills HashDecode,
    /// `needed` BufferTooSmall (the size the call reported in *out_len).
    pub fn from_status(rc: c_int, hash_len: usize, needed: u64) -> ChipError {
        match rc {
            ffi::CHIP_ERR_INVALID_ARG => ChipError::InvalidArgument,
            ffi::CHIP_ERR_BUFFER_TOO_SMALL => ChipError::BufferTooSmall(needed),
            ffi::CHIP_ERR_UNEVEN_ZFEC_CHUNKS => ChipError::UnevenZfecChunks,
            ffi::CHIP_ERR_HASH_DECODE => ChipError::HashDecode(hash_len),
            ffi::CHIP_ERR_BAO_HASH_MISMATCH => ChipError::BaoHashMismatch,
            ffi::CHIP_ERR_BAO_TRUNCATED => ChipError::BaoTruncated,
            ffi::CHIP_ERR_ZFEC => ChipError::Zfec,
            ffi::CHIP_ERR_ENCODE_ZFEC_PADDING => ChipError::EncodeZfecPadding,
            ffi::CHIP_ERR_ENCODE_INVALID_CHUNK_LENGTH => ChipError::EncodeInvalidChunkLength,
            ffi::CHIP_ERR_INVALID_VERIFIABLE_SLICE_COUNT => ChipError::InvalidVerifiableSliceCount,
            ffi::CHIP_ERR_UNSUPPORTED_FORMAT => ChipError::UnsupportedFormat,
            ffi::CHIP_ERR_UNNECESSARY_SCRUB => ChipError::UnnecessaryScrub,
            ffi::CHIP_ERR_SCRUBBED_PADDING_MISMATCH => ChipError::ScrubbedPaddingMismatch,
            ffi::CHIP_ERR_SCRUBBED_LENGTH_MISMATCH => ChipError::ScrubbedLengthMismatch,
            ffi::CHIP_ERR_INVALID_SCRUBBED_HASH => ChipError::InvalidScrubbedHash,
            ffi::CHIP_ERR_SNAP => ChipError::Snap,
            ffi::CHIP_ERR_ECIES => ChipError::Ecies,
            ffi::CHIP_ERR_SECP256K1 => ChipError::Secp256k1,
            ffi::CHIP_ERR_INVALID_HEADER_LENGTH => ChipError::InvalidHeaderLength,
            ffi::CHIP_ERR_INVALID_MAGIC => ChipError::InvalidMagic,
            ffi::CHIP_ERR_NO_DEVICE => ChipError::NoDevice(cstr(unsafe { ffi::chip_last_device_error() })),
            ffi::CHIP_ERR_DEVICE => ChipError::Device(cstr(unsafe { ffi::chip_last_device_error() })),
            s => ChipError::Other(s, cstr(unsafe { ffi::chip_strerror(s) })),
        }
    }

    /// The `chip_status` this error came from (for per-object status arrays).
    pub fn status(&self) -> c_int {
        match self {
            ChipError::InvalidArgument => ffi::CHIP_ERR_INVALID_ARG,
            ChipError::BufferTooSmall(_) => ffi::CHIP_ERR_BUFFER_TOO_SMALL,
            ChipError::UnevenZfecChunks => ffi::CHIP_ERR_UNEVEN_ZFEC_CHUNKS,
            ChipError::HashDecode(_) => ffi::CHIP_ERR_HASH_DECODE,
            ChipError::BaoHashMismatch => ffi::CHIP_ERR_BAO_HASH_MISMATCH,
            ChipError::BaoTruncated => ffi::CHIP_ERR_BAO_TRUNCATED,
            ChipError::Zfec => ffi::CHIP_ERR_ZFEC,
            ChipError::EncodeZfecPadding => ffi::CHIP_ERR_ENCODE_ZFEC_PADDING,
            ChipError::EncodeInvalidChunkLength => ffi::CHIP_ERR_ENCODE_INVALID_CHUNK_LENGTH,
            ChipError::InvalidVerifiableSliceCount => ffi::CHIP_ERR_INVALID_VERIFIABLE_SLICE_COUNT,
            ChipError::UnsupportedFormat => ffi::CHIP_ERR_UNSUPPORTED_FORMAT,
            ChipError::UnnecessaryScrub => ffi::CHIP_ERR_UNNECESSARY_SCRUB,
            ChipError::ScrubbedPaddingMismatch => ffi::CHIP_ERR_SCRUBBED_PADDING_MISMATCH,
            ChipError::ScrubbedLengthMismatch => ffi::CHIP_ERR_SCRUBBED_LENGTH_MISMATCH,
            ChipError::InvalidScrubbedHash => ffi::CHIP_ERR_INVALID_SCRUBBED_HASH,
            ChipError::Snap => ffi::CHIP_ERR_SNAP,
            ChipError::Ecies => ffi::CHIP_ERR_ECIES,
            ChipError::Secp256k1 => ffi::CHIP_ERR_SECP256K1,
            ChipError::InvalidHeaderLength => ffi::CHIP_ERR_INVALID_HEADER_LENGTH,
            ChipError::InvalidMagic => ffi::CHIP_ERR_INVALID_MAGIC,
            ChipError::NoDevice(_) => ffi::CHIP_ERR_NO_DEVICE,
            ChipError::Device(_) | ChipError::AbiMismatch(_) => ffi::CHIP_ERR_DEVICE,
            ChipError::Other(s, _) => *s,
        }
    }
}

pub type Result<T> = std::result::Result<T, ChipError>;

fn check(rc: c_int) -> Result<()> {
    if rc == ffi::CHIP_OK {
        Ok(())
    } else {
        Err(ChipError::from_status(rc, 0, 0))
    }
}

/// The loaded library must speak the ABI these declarations were written for.
fn abi() -> Result<()> {
    static ABI: OnceLock<c_int> = OnceLock::new();
    let v = *ABI.get_or_init(|| unsafe { ffi::chip_abi_version() });
    if v == ffi::CHIP_ABI_VERSION {
        Ok(())
    } else {
        Err(ChipError::AbiMismatch(v))
    }
}

/// Select the process's GPU (one process per GPU; idempotent).  Without it
/// the library follows the calling thread's current HIP device.
pub fn init(device: i32) -> Result<()> {
    abi()?;
    check(unsafe { ffi::chip_init(device) })
}

/// Run `f(out_ptr, cap, &mut out_len)` into a fresh Vec of capacity `cap`.
fn into_vec(cap: usize, hash_len: usize, f: impl FnOnce(*mut u8, u64, &mut u64) -> c_int) -> Result<Vec<u8>> {
    abi()?;
    let mut out: Vec<u8> = Vec::with_capacity(cap);
    let mut len = 0u64;
    let rc = f(out.as_mut_ptr(), cap as u64, &mut len);
    if rc != ffi::CHIP_OK {
        return Err(ChipError::from_status(rc, hash_len, len));
    }
    assert!(len as usize <= cap, "library reported {len} bytes into a {cap}-byte buffer");
    unsafe { out.set_len(len as usize) };
    Ok(out)
}

/// `into_vec`, retried once with the size a BUFFER_TOO_SMALL reported
/// (snappy output sizes are only known after decompression).
fn into_vec_grow(cap: usize, hash_len: usize, f: impl Fn(*mut u8, u64, &mut u64) -> c_int) -> Result<Vec<u8>> {
    match into_vec(cap, hash_len, &f) {
        Err(ChipError::BufferTooSmall(need)) if need as usize > cap => into_vec(need as usize, hash_len, &f),
        r => r,
    }
}

// ---- size helpers (utils.rs:47-58, bao's encoded_size) --------------------

/// utils::calc_padding_len with FEC_K generalised to k: (padding, chunk_len).
pub fn calc_padding_len(input_len: usize, k: u32) -> Result<(u32, u32)> {
    let (mut pad, mut chunk) = (0u32, 0u32);
    check(unsafe { ffi::chip_calc_padding_len(input_len as u64, k, &mut pad, &mut chunk) })?;
    Ok((pad, chunk))
}

pub fn zfec_encoded_len(input_len: usize, k: u32, m: u32) -> usize {
    unsafe { ffi::chip_zfec_encoded_len(input_len as u64, k, m) as usize }
}

pub fn bao_encoded_len(content_len: usize) -> usize {
    unsafe { ffi::chip_bao_encoded_len(content_len as u64) as usize }
}

pub fn encode_max_len(input_len: usize) -> usize {
    unsafe { ffi::chip_encode_max_len(input_len as u64) as usize }
}

// ---- the five seam functions -------------------------------------------------

/// encoding::zfec (encoding.rs:48-81): (shards [S0|..|S(m-1)], padding, chunk_len).
pub fn zfec_encode(input: &[u8], k: u32, m: u32) -> Result<(Vec<u8>, u32, u32)> {
    abi()?;
    let total = zfec_encoded_len(input.len(), k, m);
    let mut out: Vec<u8> = Vec::with_capacity(total);
    let (mut pad, mut chunk) = (0u32, 0u32);
    check(unsafe {
        ffi::chip_zfec_encode(k, m, input.as_ptr(), input.len() as u64, out.as_mut_ptr(), total as u64, &mut pad,
                              &mut chunk)
    })?;
    unsafe { out.set_len(total) };
    Ok((out, pad, chunk))
}

/// decoding::zfec (decoding.rs:35-51): shards indexed by position, as the crate does.
pub fn zfec_decode(input: &[u8], padding: u32, k: u32, m: u32) -> Result<Vec<u8>> {
    let cap = if m == 0 { 0 } else { input.len() / m as usize * k as usize };
    into_vec(cap, 0, |out, cap, len| unsafe {
        ffi::chip_zfec_decode(k, m, input.as_ptr(), input.len() as u64, padding, out, cap, len)
    })
}

/// decoding::zfec_chunks (decoding.rs:21-32) with explicit share indices
/// (`decoding::zfec_chunks` passes 0..n, the crate's positional numbering).
pub fn zfec_decode_shares(shares: &[&[u8]], idx: &[u32], padding: u32, k: u32, m: u32) -> Result<Vec<u8>> {
    if shares.len() != idx.len() {
        return Err(ChipError::InvalidArgument);
    }
    let chunk = shares.first().map_or(0, |s| s.len());
    if shares.iter().any(|s| s.len() != chunk) {
        return Err(ChipError::InvalidArgument);
    }
    let ptrs: Vec<*const u8> = shares.iter().map(|s| s.as_ptr()).collect();
    into_vec(k as usize * chunk, 0, |out, cap, len| unsafe {
        ffi::chip_zfec_decode_shares(k, m, ptrs.as_ptr(), idx.as_ptr(), shares.len() as u32, chunk as u64, padding,
                                     out, cap, len)
    })
}

/// encoding::bao (encoding.rs:38-44): the combined pre-order stream and its root hash.
pub fn bao_encode(input: &[u8]) -> Result<(Vec<u8>, [u8; HASH_LEN])> {
    let mut hash = [0u8; HASH_LEN];
    let enc = into_vec(bao_encoded_len(input.len()), 0, |out, cap, len| unsafe {
        ffi::chip_bao_encode(input.as_ptr(), input.len() as u64, out, cap, len, hash.as_mut_ptr())
    })?;
    Ok((enc, hash))
}

/// decoding::bao (decoding.rs:53-60): every node verified, the content returned.
pub fn bao_decode(input: &[u8], hash: &[u8]) -> Result<Vec<u8>> {
    into_vec(input.len(), hash.len(), |out, cap, len| unsafe {
        ffi::chip_bao_decode(input.as_ptr(), input.len() as u64, hash.as_ptr(), hash.len() as u64, out, cap, len)
    })
}

/// BLAKE3 of `input` (== the bao root hash), computed on the device.
pub fn blake3(input: &[u8]) -> Result<[u8; HASH_LEN]> {
    abi()?;
    let mut hash = [0u8; HASH_LEN];
    check(unsafe { ffi::chip_blake3(input.as_ptr(), input.len() as u64, hash.as_mut_ptr()) })?;
    Ok(hash)
}

// ---- slices and scrub (decoding.rs:116-212) -------------------------------

/// extract_slice (decoding.rs:116-127) with a u64 index (the crate's u16
/// `index * SLICE_LEN` wraps at index 64).
pub fn extract_slice(encoded: &[u8], index: u64) -> Result<Vec<u8>> {
    let content = encoded_content_len(encoded)?;
    let cap = unsafe { ffi::chip_bao_slice_len(content, index * ffi::CHIP_SLICE_LEN as u64, ffi::CHIP_SLICE_LEN as u64) };
    into_vec(cap as usize, 0, |out, cap, len| unsafe {
        ffi::chip_bao_extract_slice(encoded.as_ptr(), encoded.len() as u64, index, ffi::CHIP_SLICE_LEN as u64, out,
                                    cap, len)
    })
}

/// verify_slice (decoding.rs:129-149): `count` 1 KiB slices from `index`, verified.
pub fn verify_slice(hash: &[u8], input: &[u8], index: u64, count: u64) -> Result<Vec<u8>> {
    let cap = (count as usize).saturating_mul(ffi::CHIP_SLICE_LEN).min(input.len());
    into_vec(cap, hash.len(), |out, cap, len| unsafe {
        ffi::chip_bao_verify_slice(hash.as_ptr(), hash.len() as u64, input.as_ptr(), input.len() as u64, index, count,
                                   out, cap, len)
    })
}

/// scrub (decoding.rs:151-212), decoding the good shards with their TRUE
/// indices.  An intact stream is `Err(ChipError::UnnecessaryScrub)`.
pub fn scrub(input: &[u8], hash: &[u8], padding: u32, chunk_len: u32) -> Result<Vec<u8>> {
    into_vec(input.len(), hash.len(), |out, cap, len| unsafe {
        ffi::chip_scrub(input.as_ptr(), input.len() as u64, hash.as_ptr(), hash.len() as u64, padding, chunk_len,
                        out, cap, len)
    })
}

fn encoded_content_len(encoded: &[u8]) -> Result<u64> {
    let head: [u8; 8] = encoded.get(..8).and_then(|h| h.try_into().ok()).ok_or(ChipError::BaoTruncated)?;
    Ok(u64::from_le_bytes(head))
}

// ---- host stages (encoding.rs:16-36, decoding.rs:62-77) ---------------------

/// The two values ecies::encrypt draws from thread_rng, for bit-exact tests;
/// production code passes `None` (fresh random values, as the crate).
#[derive(Clone, Copy, Debug)]
pub struct EciesInject<'a> {
    pub ephemeral_sk: &'a [u8; 32],
    pub nonce: &'a [u8; 16],
}

fn inject_ptr(inject: Option<EciesInject<'_>>, slot: &mut ffi::chip_ecies_inject) -> *const ffi::chip_ecies_inject {
    match inject {
        None => ptr::null(),
        Some(i) => {
            *slot = ffi::chip_ecies_inject { ephemeral_sk: i.ephemeral_sk.as_ptr(), nonce: i.nonce.as_ptr() };
            slot
        }
    }
}

pub fn snap_compress(input: &[u8]) -> Result<Vec<u8>> {
    let cap = unsafe { ffi::chip_snap_max_len(input.len() as u64) } as usize;
    into_vec(cap, 0, |out, cap, len| unsafe {
        ffi::chip_snap_compress(input.as_ptr(), input.len() as u64, out, cap, len)
    })
}

pub fn snap_decompress(input: &[u8]) -> Result<Vec<u8>> {
    into_vec_grow(input.len().saturating_mul(2).max(1024), 0, |out, cap, len| unsafe {
        ffi::chip_snap_decompress(input.as_ptr(), input.len() as u64, out, cap, len)
    })
}

pub fn ecies_encrypt(pubkey: &[u8], input: &[u8], inject: Option<EciesInject<'_>>) -> Result<Vec<u8>> {
    let mut slot = ffi::chip_ecies_inject { ephemeral_sk: ptr::null(), nonce: ptr::null() };
    let inj = inject_ptr(inject, &mut slot);
    into_vec(input.len() + 97, 0, |out, cap, len| unsafe {
        ffi::chip_ecies_encrypt(pubkey.as_ptr(), pubkey.len() as u64, inj, input.as_ptr(), input.len() as u64, out,
                                cap, len)
    })
}

pub fn ecies_decrypt(input: &[u8], secret_key: &[u8]) -> Result<Vec<u8>> {
    into_vec(input.len(), 0, |out, cap, len| unsafe {
        ffi::chip_ecies_decrypt(secret_key.as_ptr(), secret_key.len() as u64, input.as_ptr(), input.len() as u64,
                                out, cap, len)
    })
}

// ---- encode() / decode() glue (encoding.rs:86-172, decoding.rs:80-114) ------

/// encoding::encode: (stream, hash, EncodeInfo), the crate's `Encoded`.
pub fn encode(pubkey: &[u8], input: &[u8], format: u8, inject: Option<EciesInject<'_>>)
              -> Result<(Vec<u8>, [u8; HASH_LEN], ChipEncodeInfo)> {
    let mut hash = [0u8; HASH_LEN];
    let mut info = ChipEncodeInfo::default();
    let mut slot = ffi::chip_ecies_inject { ephemeral_sk: ptr::null(), nonce: ptr::null() };
    let inj = inject_ptr(inject, &mut slot);
    let out = into_vec(encode_max_len(input.len()), 0, |out, cap, len| unsafe {
        ffi::chip_encode(format, pubkey.as_ptr(), pubkey.len() as u64, inj, input.as_ptr(), input.len() as u64, out,
                         cap, len, hash.as_mut_ptr(), &mut info)
    })?;
    Ok((out, hash, info))
}

/// decoding::decode: bao -> zfec on the device, ecies -> snap on the host.
pub fn decode(secret_key: &[u8], hash: &[u8], input: &[u8], padding: u32, format: u8) -> Result<Vec<u8>> {
    into_vec_grow(input.len().max(1024), hash.len(), |out, cap, len| unsafe {
        ffi::chip_decode(secret_key.as_ptr(), secret_key.len() as u64, hash.as_ptr(), hash.len() as u64,
                         input.as_ptr(), input.len() as u64, padding, format, out, cap, len)
    })
}

// ---- flat-file container (file.rs) ---------------------------------------

/// Header::new (file.rs:263-289).  `aux` = the signature's auxiliary
/// randomness (None = fresh, as the crate).
#[allow(clippy::too_many_arguments)]
pub fn header_new(sk: &[u8], pk: &[u8], hash: &[u8], format: u8, chunk_index: u8, encoded_len: u32,
                  padding_len: u32, metadata: Option<&[u8; 8]>, aux: Option<&[u8; 32]>) -> Result<ChipHeader> {
    abi()?;
    let mut h = ChipHeader::default();
    check(unsafe {
        ffi::chip_header_new(sk.as_ptr(), sk.len() as u64, pk.as_ptr(), pk.len() as u64, hash.as_ptr(),
                             hash.len() as u64, format, chunk_index, encoded_len, padding_len,
                             metadata.map_or(ptr::null(), |m| m.as_ptr()), aux.map_or(ptr::null(), |a| a.as_ptr()),
                             &mut h)
    })?;
    Ok(h)
}

/// Header::try_to_vec (file.rs:292-335).
pub fn header_to_bytes(h: &ChipHeader) -> Result<[u8; ffi::CHIP_HEADER_LEN]> {
    let mut out = [0u8; ffi::CHIP_HEADER_LEN];
    check(unsafe { ffi::chip_header_to_bytes(h, out.as_mut_ptr()) })?;
    Ok(out)
}

/// Header::try_from(&[u8]) (file.rs:116-154); a short slice is an error, not a panic.
pub fn header_parse(bytes: &[u8]) -> Result<ChipHeader> {
    let mut h = ChipHeader::default();
    check(unsafe { ffi::chip_header_parse(bytes.as_ptr(), bytes.len() as u64, &mut h) })?;
    Ok(h)
}

/// file::encode (file.rs:409-440): header || encode(pubkey, input, level).
pub fn file_encode(sk: &[u8], pk: Option<&[u8]>, input: &[u8], level: u8, metadata: Option<&[u8; 8]>)
                   -> Result<(Vec<u8>, ChipEncodeInfo)> {
    let mut info = ChipEncodeInfo::default();
    let (pkp, pkl) = pk.map_or((ptr::null(), 0u64), |p| (p.as_ptr(), p.len() as u64));
    let out = into_vec(ffi::CHIP_HEADER_LEN + encode_max_len(input.len()), 0, |out, cap, len| unsafe {
        ffi::chip_file_encode(sk.as_ptr(), sk.len() as u64, pkp, pkl, input.as_ptr(), input.len() as u64, level,
                              metadata.map_or(ptr::null(), |m| m.as_ptr()), ptr::null(), ptr::null(), out, cap, len,
                              &mut info)
    })?;
    Ok((out, info))
}

/// file::decode (file.rs:395-407): (header, decoded content).
pub fn file_decode(sk: &[u8], input: &[u8]) -> Result<(ChipHeader, Vec<u8>)> {
    let mut hdr = ChipHeader::default();
    let hdrp: *mut ChipHeader = &mut hdr; // the retry closure must be Fn
    let out = into_vec_grow(input.len().max(1024), 0, |out, cap, len| unsafe {
        ffi::chip_file_decode(sk.as_ptr(), sk.len() as u64, input.as_ptr(), input.len() as u64, hdrp, out, cap, len)
    })?;
    Ok((hdr, out))
}

// ---- streaming hasher (utils.rs:104-137) ----------------------------------

/// utils::BaoHasher: appends land in HBM, chunk CVs are hashed as whole
/// units arrive; `finalize` lays the stream out and builds the parents.
pub struct BaoHasher(*mut ffi::chip_bao_hasher);

// the library serialises every call on one hasher with its own mutex
unsafe impl Send for BaoHasher {}
unsafe impl Sync for BaoHasher {}

impl BaoHasher {
    pub fn new() -> Result<BaoHasher> {
        abi()?;
        let mut h = ptr::null_mut();
        check(unsafe { ffi::chip_bao_hasher_new(&mut h) })?;
        Ok(BaoHasher(h))
    }

    /// The bytes are copied before this returns.
    pub fn update(&self, buf: &[u8]) -> Result<()> {
        check(unsafe { ffi::chip_bao_hasher_update(self.0, buf.as_ptr(), buf.len() as u64) })
    }

    pub fn finalize(&self) -> Result<[u8; HASH_LEN]> {
        let mut hash = [0u8; HASH_LEN];
        check(unsafe { ffi::chip_bao_hasher_finalize(self.0, hash.as_mut_ptr()) })?;
        Ok(hash)
    }

    pub fn len(&self) -> u64 {
        unsafe { ffi::chip_bao_hasher_len(self.0) }
    }

    pub fn is_empty(&self) -> bool {
        self.len() == 0
    }

    /// The combined bao encoding (after `finalize`).
    pub fn read_all(&self) -> Result<Vec<u8>> {
        let cap = bao_encoded_len(self.len() as usize);
        into_vec(cap, 0, |out, cap, len| unsafe { ffi::chip_bao_hasher_read_all(self.0, out, cap, len) })
    }
}

impl Drop for BaoHasher {
    fn drop(&mut self) {
        unsafe { ffi::chip_bao_hasher_free(self.0) }
    }
}

/// Destroy every parked (freed, kept for reuse) hasher; returns the device
/// bytes freed.  Parked hashers hold at most CHIP_HASHER_PARK_MIB (3 GiB).
pub fn drop_hasher_cache() -> u64 {
    unsafe { ffi::chip_bao_hasher_drop_cache() }
}

/// Device bytes the parked hashers hold.
pub fn hasher_cached_bytes() -> u64 {
    unsafe { ffi::chip_bao_hasher_cached_bytes() }
}

/// Where this process's host-copy path sits on the box (JSON): the GPU's
/// NUMA node, the staging ring's node, the copy workers' nodes (diagnostic).
pub fn host_topology() -> Result<String> {
    abi()?;
    let mut len = 0u64;
    let _ = unsafe { ffi::chip_host_topology(ptr::null_mut(), 0, &mut len) };
    let mut buf = vec![0u8; len.max(1) as usize];
    check(unsafe { ffi::chip_host_topology(buf.as_mut_ptr() as *mut std::os::raw::c_char, len, &mut len) })?;
    buf.truncate(len.saturating_sub(1) as usize);
    Ok(String::from_utf8_lossy(&buf).into_owned())
}

// ---- device-resident batch API ----------------------------------------------

/// A HIP stream handle (`hipStream_t`); [`Stream::DEFAULT`] = the library's
/// per-thread stream.  The batch calls enqueue on it and return.  The handle
/// is private: safe code gets only [`Stream::DEFAULT`]; a caller's own stream
/// comes in through [`Stream::from_raw`], whose caller vouches for it.
#[derive(Clone, Copy, Debug)]
pub struct Stream(*mut c_void);

impl Stream {
    pub const DEFAULT: Stream = Stream(ptr::null_mut());

    /// # Safety
    /// `raw` must be a live `hipStream_t` of the device the library runs on,
    /// and stay alive until the work enqueued on it through this handle has
    /// finished.
    pub unsafe fn from_raw(raw: *mut c_void) -> Stream {
        Stream(raw)
    }

    pub fn as_raw(&self) -> *mut c_void {
        self.0
    }
}

unsafe impl Send for Stream {}
unsafe impl Sync for Stream {}

/// Device memory from `chip_device_alloc`: class-balanced from 1 GiB up
/// (DESIGN.md §2), contiguous below.  Freed on drop.
pub struct DeviceBuffer {
    ptr: *mut c_void,
    len: usize,
}

unsafe impl Send for DeviceBuffer {}
unsafe impl Sync for DeviceBuffer {}

impl DeviceBuffer {
    pub fn new(bytes: usize) -> Result<DeviceBuffer> {
        abi()?;
        let mut p = ptr::null_mut();
        check(unsafe { ffi::chip_device_alloc(bytes as u64, &mut p) })?;
        Ok(DeviceBuffer { ptr: p, len: bytes })
    }

    pub fn len(&self) -> usize {
        self.len
    }

    pub fn is_empty(&self) -> bool {
        self.len == 0
    }

    pub fn as_ptr(&self) -> *const u8 {
        self.ptr as *const u8
    }

    pub fn as_mut_ptr(&mut self) -> *mut u8 {
        self.ptr as *mut u8
    }

    /// (memory classes found, classes used, seconds) of a class-balanced buffer.
    pub fn alloc_info(&self) -> Result<(u32, u32, f64)> {
        let (mut f, mut u, mut s) = (0u32, 0u32, 0f64);
        check(unsafe { ffi::chip_device_alloc_info(self.ptr, &mut f, &mut u, &mut s) })?;
        Ok((f, u, s))
    }
}

impl Drop for DeviceBuffer {
    fn drop(&mut self) {
        if !self.ptr.is_null() {
            unsafe { ffi::chip_device_free(self.ptr) };
        }
    }
}

enum Mem {
    Owned(DeviceBuffer),
    Borrowed(*mut u8, usize),
}

/// `count` rows of `row` bytes at a 16-B multiple `stride` (256-B from `alloc`) in device memory:
/// the shape every batch entry point takes (object o at base + o * stride).
pub struct DeviceRows {
    mem: Mem,
    pub count: u64,
    pub row: u64,
    pub stride: u64,
    off: u64, // where row 0 starts in `mem` (alloc_streams: STREAM_OFFSET)
}

/// Where `DeviceRows::alloc_streams` puts each bao stream in its row: after
/// the stream's 8-byte header every chunk and parent node then starts on a
/// 64-B boundary, which runs level 12 4-11 % and decode 4-12 % faster than
/// streams at the row start.
pub const STREAM_OFFSET: u64 = 56;

unsafe impl Send for DeviceRows {}

impl DeviceRows {
    /// Allocate through `chip_device_alloc` (the default: the fast placement).
    pub fn alloc(count: u64, row: u64) -> Result<DeviceRows> {
        // 256-B pitch: every row's 128-B pieces start on a memory line (a 16-B pitch
        // costs the kernels 1.21x the read traffic)
        let stride = (row + 255) / 256 * 256;
        let buf = DeviceBuffer::new((count * stride).max(16) as usize)?;
        Ok(DeviceRows { mem: Mem::Owned(buf), count, row, stride, off: 0 })
    }

    /// Rows for the bao streams of `content_len`-byte contents (the output of
    /// `encode_batch` at Zfec|Bao with content 8 * chunk_len, or of
    /// `bao_encode_batch`), each stream STREAM_OFFSET bytes into its row when
    /// it has more than 512 chunks (the entry points take those at any 8-B
    /// phase; smaller streams stay at the row start).
    pub fn alloc_streams(count: u64, content_len: u64) -> Result<DeviceRows> {
        let len = bao_encoded_len(content_len as usize) as u64;
        let off = if content_len > 512 * 1024 { STREAM_OFFSET } else { 0 };
        let stride = (off + len + 255) / 256 * 256;
        let buf = DeviceBuffer::new((count * stride).max(16) as usize)?;
        Ok(DeviceRows { mem: Mem::Owned(buf), count, row: len, stride, off })
    }

    /// Wrap caller-owned device memory (any 16-B aligned allocation works,
    /// only slower than `alloc`'s).
    ///
    /// # Safety
    /// `base` must point to at least `(count - 1) * stride + row` bytes of
    /// device memory that outlive the returned value.
    pub unsafe fn from_raw(base: *mut u8, count: u64, row: u64, stride: u64) -> Result<DeviceRows> {
        if base as usize % 16 != 0 || stride % 16 != 0 || (count > 1 && stride < row) {
            return Err(ChipError::InvalidArgument);
        }
        let bytes = if count == 0 { 0 } else { ((count - 1) * stride + row) as usize };
        Ok(DeviceRows { mem: Mem::Borrowed(base, bytes), count, row, stride, off: 0 })
    }

    /// Bytes from row 0's start to the end of the memory.
    fn bytes(&self) -> usize {
        let total = match &self.mem {
            Mem::Owned(b) => b.len(),
            Mem::Borrowed(_, n) => *n,
        };
        total.saturating_sub(self.off as usize)
    }

    /// Row 0's first byte.
    pub fn as_ptr(&self) -> *const u8 {
        let base = match &self.mem {
            Mem::Owned(b) => b.as_ptr(),
            Mem::Borrowed(p, _) => *p as *const u8,
        };
        base.wrapping_add(self.off as usize)
    }

    pub fn as_mut_ptr(&mut self) -> *mut u8 {
        let off = self.off as usize;
        let base = match &mut self.mem {
            Mem::Owned(b) => b.as_mut_ptr(),
            Mem::Borrowed(p, _) => *p,
        };
        base.wrapping_add(off)
    }

    /// The rows hold `count` objects of at least `row` bytes each.
    fn holds(&self, count: u64, row: u64) -> Result<()> {
        let need = if count == 0 { 0 } else { (count - 1) * self.stride + row };
        if count > self.count || row > self.stride.max(self.row) || need as usize > self.bytes() {
            return Err(ChipError::InvalidArgument);
        }
        Ok(())
    }
}

/// Scratch of a batch call, sized by the matching `*_scratch_len`.
pub fn scratch(bytes: u64) -> Result<DeviceBuffer> {
    DeviceBuffer::new(bytes.max(16) as usize)
}

/// zfec k-of-m encode of `input.count` objects of `n` bytes (encoding.rs:48-81
/// per object): object o's m shards to row o of `out`.
pub fn zfec_encode_batch(k: u32, m: u32, input: &DeviceRows, n: u64, out: &mut DeviceRows, stream: Stream)
                         -> Result<()> {
    input.holds(input.count, n)?;
    out.holds(input.count, zfec_encoded_len(n as usize, k, m) as u64)?;
    check(unsafe {
        ffi::chip_zfec_encode_batch_dev(k, m, input.as_ptr(), input.stride, n, input.count, out.as_mut_ptr(),
                                        out.stride, stream.0)
    })
}

/// Erasure decode (decoding.rs:21-51 with true indices): `idx` names the
/// shares present in each row of `input` (shard i at i * chunk_len), the
/// k * chunk_len data bytes of object o go to row o of `out`.
pub fn zfec_decode_batch(k: u32, m: u32, input: &DeviceRows, chunk_len: u64, idx: &[u32], out: &mut DeviceRows,
                         stream: Stream) -> Result<()> {
    input.holds(input.count, m as u64 * chunk_len)?;
    out.holds(input.count, k as u64 * chunk_len)?;
    check(unsafe {
        ffi::chip_zfec_decode_batch_dev(k, m, input.as_ptr(), input.stride, chunk_len, idx.as_ptr(),
                                        idx.len() as u32, input.count, out.as_mut_ptr(), out.stride, stream.0)
    })
}

/// bao encode of every row (encoding.rs:38-44): streams to `out`, hashes to
/// `hashes` (count * 32 bytes).  `scratch`: [`bao_scratch_len`] bytes.
pub fn bao_encode_batch(input: &DeviceRows, n: u64, out: &mut DeviceRows, hashes: &mut DeviceBuffer,
                        scratch: &mut DeviceBuffer, stream: Stream) -> Result<()> {
    input.holds(input.count, n)?;
    out.holds(input.count, bao_encoded_len(n as usize) as u64)?;
    if hashes.len() < input.count as usize * HASH_LEN || (scratch.len() as u64) < bao_scratch_len(n, input.count) {
        return Err(ChipError::InvalidArgument);
    }
    check(unsafe {
        ffi::chip_bao_encode_batch_dev(input.as_ptr(), input.stride, n, input.count, out.as_mut_ptr(), out.stride,
                                       hashes.as_mut_ptr(), scratch.ptr, stream.0)
    })
}

pub fn bao_scratch_len(n: u64, count: u64) -> u64 {
    unsafe { ffi::chip_bao_scratch_len(n, count) }
}

/// bao verify-decode of every row (decoding.rs:53-60): content to `out`,
/// per-object status (u32, 0 or a chip_status) to `status` (count * 4 bytes).
pub fn bao_decode_batch(input: &DeviceRows, n: u64, hashes: &DeviceBuffer, out: &mut DeviceRows,
                        status: &mut DeviceBuffer, scratch: &mut DeviceBuffer, stream: Stream) -> Result<()> {
    input.holds(input.count, bao_encoded_len(n as usize) as u64)?;
    out.holds(input.count, n)?;
    if hashes.len() < input.count as usize * HASH_LEN || status.len() < input.count as usize * 4 ||
        (scratch.len() as u64) < bao_scratch_len(n, input.count) {
        return Err(ChipError::InvalidArgument);
    }
    check(unsafe {
        ffi::chip_bao_decode_batch_dev(input.as_ptr(), input.stride, n, input.count, hashes.as_ptr(),
                                       out.as_mut_ptr(), out.stride, status.as_mut_ptr() as *mut u32, scratch.ptr,
                                       stream.0)
    })
}

pub fn encode_scratch_len(format: u8, n: u64, count: u64) -> u64 {
    unsafe { ffi::chip_encode_scratch_len(format, n, count) }
}

pub fn decode_scratch_len(format: u8, in_len: u64, count: u64) -> u64 {
    unsafe { ffi::chip_decode_scratch_len(format, in_len, count) }
}

/// encode() (encoding.rs:86-172) of every row at a device-only level (Bao
/// and/or Zfec bits; Zfec|Bao runs fused).  Returns (encoded length, EncodeInfo).
pub fn encode_batch(format: u8, input: &DeviceRows, n: u64, out: &mut DeviceRows, hashes: &mut DeviceBuffer,
                    scratch: &mut DeviceBuffer, stream: Stream) -> Result<(u64, ChipEncodeInfo)> {
    input.holds(input.count, n)?;
    if hashes.len() < input.count as usize * HASH_LEN ||
        (scratch.len() as u64) < encode_scratch_len(format, n, input.count) {
        return Err(ChipError::InvalidArgument);
    }
    let mut out_len = 0u64;
    let mut info = ChipEncodeInfo::default();
    check(unsafe {
        ffi::chip_encode_batch_dev(format, input.as_ptr(), input.stride, n, input.count, out.as_mut_ptr(),
                                   out.stride, &mut out_len, hashes.as_mut_ptr(), &mut info, scratch.ptr, stream.0)
    })?;
    Ok((out_len, info))
}

/// decode() (decoding.rs:80-114) of every row at a device-only level; per-object
/// status (u32) to `status`.  Returns the decoded length.
#[allow(clippy::too_many_arguments)]
pub fn decode_batch(format: u8, input: &DeviceRows, in_len: u64, hashes: &DeviceBuffer, padding: u32,
                    out: &mut DeviceRows, status: &mut DeviceBuffer, scratch: &mut DeviceBuffer, stream: Stream)
                    -> Result<u64> {
    input.holds(input.count, in_len)?;
    if hashes.len() < input.count as usize * HASH_LEN || status.len() < input.count as usize * 4 ||
        (scratch.len() as u64) < decode_scratch_len(format, in_len, input.count) {
        return Err(ChipError::InvalidArgument);
    }
    let mut out_len = 0u64;
    check(unsafe {
        ffi::chip_decode_batch_dev(format, input.as_ptr(), input.stride, in_len, input.count, hashes.as_ptr(), padding,
                                   out.as_mut_ptr(), out.stride, &mut out_len, status.as_mut_ptr() as *mut u32,
                                   scratch.ptr, stream.0)
    })?;
    Ok(out_len)
}

fn abi_ext() -> Result<()> {
    abi()?;
    match unsafe { ffi_ext::chipx_abi_version() } {
        ffi_ext::CHIPX_ABI_VERSION => Ok(()),
        v => Err(ChipError::AbiMismatch(v)),
    }
}

/// Where [`encode_ragged`]'s caller should put each object in one output
/// buffer (host only): (out_off, out_len, total bytes).
pub fn ragged_layout(format: u8, sizes: &[u64], align: u64, stream_offset: u64) -> Result<(Vec<u64>, Vec<u64>, u64)> {
    let (mut off, mut len, mut total) = (vec![0u64; sizes.len()], vec![0u64; sizes.len()], 0u64);
    check(unsafe {
        ffi_ext::chipx_ragged_layout(format, sizes.as_ptr(), sizes.len() as u64, align, stream_offset, off.as_mut_ptr(),
                                     len.as_mut_ptr(), &mut total)
    })?;
    Ok((off, len, total))
}

pub fn ragged_scratch_len(format: u8, lens: &[u64], decode: bool) -> u64 {
    unsafe { ffi_ext::chipx_ragged_scratch_len(format, lens.as_ptr(), lens.len() as u64, decode as c_int) }
}

/// encode() at a device-only level of objects of DIFFERENT lengths in one
/// call (include/carbonado_hip_ext.h): object o = `input[in_off[o]..][..sizes[o]]`
/// into `out[out_off[o]..]`, its hash to `hashes[32 o..]`.  Returns the encoded
/// length and EncodeInfo of every object.  Enqueued on `stream`, not synchronised.
#[allow(clippy::too_many_arguments)]
pub fn encode_ragged(format: u8, input: &DeviceBuffer, in_off: &[u64], sizes: &[u64], out: &mut DeviceBuffer,
                     out_off: &[u64], hashes: &mut DeviceBuffer, scratch: &mut DeviceBuffer, stream: Stream)
                     -> Result<(Vec<u64>, Vec<ChipEncodeInfo>)> {
    let count = sizes.len();
    if in_off.len() != count || out_off.len() != count || hashes.len() < count * HASH_LEN ||
        (scratch.len() as u64) < ragged_scratch_len(format, sizes, false) ||
        in_off.iter().zip(sizes).any(|(&o, &n)| o + n > input.len() as u64) {
        return Err(ChipError::InvalidArgument);
    }
    let (_, need, _) = ragged_layout(format, sizes, 256, 0)?;
    if out_off.iter().zip(&need).any(|(&o, &l)| o + l > out.len() as u64) {
        return Err(ChipError::InvalidArgument);
    }
    abi_ext()?;
    let mut lens = vec![0u64; count];
    let mut infos = vec![ChipEncodeInfo::default(); count];
    check(unsafe {
        ffi_ext::chipx_encode_ragged_dev(format, input.as_ptr(), in_off.as_ptr(), sizes.as_ptr(), count as u64,
                                         out.as_mut_ptr(), out_off.as_ptr(), lens.as_mut_ptr(), hashes.as_mut_ptr(),
                                         infos.as_mut_ptr(), scratch.ptr, stream.0)
    })?;
    Ok((lens, infos))
}

/// decode() of encodings of different lengths in one call; the per-object
/// status (u32: 0 or 5 = hash mismatch) goes to `status` on the device.
/// Returns the decoded lengths.  The bounds check is made before the lengths
/// are known: `out` must hold `in_len[o]` bytes from `out_off[o]` (a decoding
/// is never longer than its encoding).
#[allow(clippy::too_many_arguments)]
pub fn decode_ragged(format: u8, input: &DeviceBuffer, in_off: &[u64], in_len: &[u64], hashes: &DeviceBuffer,
                     padding: &[u32], out: &mut DeviceBuffer, out_off: &[u64], status: &mut DeviceBuffer,
                     scratch: &mut DeviceBuffer, stream: Stream) -> Result<Vec<u64>> {
    let count = in_len.len();
    if in_off.len() != count || out_off.len() != count || padding.len() != count ||
        hashes.len() < count * HASH_LEN || status.len() < count * 4 ||
        (scratch.len() as u64) < ragged_scratch_len(format, in_len, true) ||
        in_off.iter().zip(in_len).any(|(&o, &l)| o + l > input.len() as u64) ||
        // a decoding is never longer than its encoding
        out_off.iter().zip(in_len).any(|(&o, &l)| o + l > out.len() as u64) {
        return Err(ChipError::InvalidArgument);
    }
    abi_ext()?;
    let mut lens = vec![0u64; count];
    check(unsafe {
        ffi_ext::chipx_decode_ragged_dev(format, input.as_ptr(), in_off.as_ptr(), in_len.as_ptr(), count as u64,
                                         hashes.as_ptr(), padding.as_ptr(), out.as_mut_ptr(), out_off.as_ptr(),
                                         lens.as_mut_ptr(), status.as_mut_ptr() as *mut u32, scratch.ptr, stream.0)
    })?;
    Ok(lens)
}

fn abi_audit() -> Result<()> {
    abi()?;
    match unsafe { ffi_audit::chipa_abi_version() } {
        ffi_audit::CHIPA_ABI_VERSION => Ok(()),
        v => Err(ChipError::AbiMismatch(v)),
    }
}

/// The sizes and places of every slice request's proof and content (host
/// only; include/carbonado_hip_audit.h).
#[derive(Debug, Clone, Default)]
pub struct SliceLayout {
    pub proof_off: Vec<u64>,
    pub proof_len: Vec<u64>,
    pub content_off: Vec<u64>,
    pub content_len: Vec<u64>,
    pub proof_total: u64,
    pub content_total: u64,
}

/// `content_len[r]` = the content length of request r's stream; request r is
/// slices `[index[r], index[r] + count[r])` of 1024 bytes.
pub fn slice_layout(content_len: &[u64], index: &[u64], count: &[u64], align: u64) -> Result<SliceLayout> {
    let nreq = content_len.len();
    if index.len() != nreq || count.len() != nreq {
        return Err(ChipError::InvalidArgument);
    }
    let mut l = SliceLayout { proof_off: vec![0; nreq], proof_len: vec![0; nreq], content_off: vec![0; nreq],
                              content_len: vec![0; nreq], proof_total: 0, content_total: 0 };
    check(unsafe {
        ffi_audit::chipa_slice_layout(content_len.as_ptr(), index.as_ptr(), count.as_ptr(), nreq as u64, align,
                                      l.proof_off.as_mut_ptr(), l.proof_len.as_mut_ptr(), l.content_off.as_mut_ptr(),
                                      l.content_len.as_mut_ptr(), &mut l.proof_total, &mut l.content_total)
    })?;
    Ok(l)
}

pub fn audit_scratch_len(nstreams: u64, nreq: u64) -> u64 {
    unsafe { ffi_audit::chipa_audit_scratch_len(nstreams, nreq) }
}

/// extract_slice of every request from device-resident bao streams: request
/// r's proof (stream `req_stream[r]` = `streams[in_off[s]..][..in_len[s]]`,
/// slices `[index[r], index[r] + count[r])`) into `proofs[proof_off[r]..][..proof_len[r]]`,
/// offsets and exact lengths as [`slice_layout`] gives them.  No hashing.
/// Enqueued on `stream`, not synchronised.
#[allow(clippy::too_many_arguments)]
pub fn extract_slices(streams: &DeviceBuffer, in_off: &[u64], in_len: &[u64], req_stream: &[u32], index: &[u64],
                      count: &[u64], proofs: &mut DeviceBuffer, proof_off: &[u64], proof_len: &[u64],
                      scratch: &mut DeviceBuffer, stream: Stream) -> Result<()> {
    let (nstreams, nreq) = (in_len.len(), req_stream.len());
    if in_off.len() != nstreams || index.len() != nreq || count.len() != nreq || proof_off.len() != nreq ||
        proof_len.len() != nreq || (scratch.len() as u64) < audit_scratch_len(nstreams as u64, nreq as u64) ||
        in_off.iter().zip(in_len).any(|(&o, &l)| o + l > streams.len() as u64) ||
        proof_off.iter().zip(proof_len).any(|(&o, &l)| o + l > proofs.len() as u64) {
        return Err(ChipError::InvalidArgument);
    }
    abi_audit()?;
    check(unsafe {
        ffi_audit::chipa_extract_slices_dev(streams.as_ptr(), in_off.as_ptr(), in_len.as_ptr(), nstreams as u64,
                                            req_stream.as_ptr(), index.as_ptr(), count.as_ptr(), nreq as u64,
                                            proofs.as_mut_ptr(), proof_off.as_ptr(), proof_len.as_ptr(), scratch.ptr,
                                            stream.0)
    })
}

/// verify_slice of every request straight from the resident streams
/// (`hashes[32 s..]` = stream s's hash): the per-request status (u32: 0 or 5 =
/// hash mismatch) goes to `status` on the device, the content of request r to
/// `content[content_off[r]..]` where its status is 0 and zeros otherwise.
/// Returns the content lengths.  The bounds check is made before they are
/// known: `content` must hold `count[r] * 1024` bytes from `content_off[r]`.
#[allow(clippy::too_many_arguments)]
pub fn verify_slices(streams: &DeviceBuffer, in_off: &[u64], in_len: &[u64], hashes: &DeviceBuffer,
                     req_stream: &[u32], index: &[u64], count: &[u64], content: &mut DeviceBuffer,
                     content_off: &[u64], status: &mut DeviceBuffer, scratch: &mut DeviceBuffer, stream: Stream)
                     -> Result<Vec<u64>> {
    let (nstreams, nreq) = (in_len.len(), req_stream.len());
    if in_off.len() != nstreams || index.len() != nreq || count.len() != nreq || content_off.len() != nreq ||
        hashes.len() < nstreams * HASH_LEN || status.len() < nreq * 4 ||
        (scratch.len() as u64) < audit_scratch_len(nstreams as u64, nreq as u64) ||
        in_off.iter().zip(in_len).any(|(&o, &l)| o + l > streams.len() as u64) ||
        content_off.iter().zip(count).any(|(&o, &c)| c > (1 << 53) || o + c * 1024 > content.len() as u64) {
        return Err(ChipError::InvalidArgument);
    }
    abi_audit()?;
    let mut lens = vec![0u64; nreq];
    check(unsafe {
        ffi_audit::chipa_verify_slices_dev(streams.as_ptr(), in_off.as_ptr(), in_len.as_ptr(), hashes.as_ptr(),
                                           nstreams as u64, req_stream.as_ptr(), index.as_ptr(), count.as_ptr(),
                                           nreq as u64, content.as_mut_ptr(), content_off.as_ptr(), lens.as_mut_ptr(),
                                           status.as_mut_ptr() as *mut u32, scratch.ptr, stream.0)
    })?;
    Ok(lens)
}

/// The auditor's side of [`verify_slices`]: the same verdict and content from
/// the proofs [`extract_slices`] wrote, without the streams.  `content_len[r]`
/// = the content length of the stream request r's proof came from,
/// `hashes[32 r..]` that stream's hash (one per request).
#[allow(clippy::too_many_arguments)]
pub fn verify_slice_proofs(proofs: &DeviceBuffer, proof_off: &[u64], proof_len: &[u64], content_len: &[u64],
                           hashes: &DeviceBuffer, index: &[u64], count: &[u64], content: &mut DeviceBuffer,
                           content_off: &[u64], status: &mut DeviceBuffer, scratch: &mut DeviceBuffer, stream: Stream)
                           -> Result<Vec<u64>> {
    let nreq = proof_len.len();
    if proof_off.len() != nreq || content_len.len() != nreq || index.len() != nreq || count.len() != nreq ||
        content_off.len() != nreq || hashes.len() < nreq * HASH_LEN || status.len() < nreq * 4 ||
        (scratch.len() as u64) < audit_scratch_len(nreq as u64, nreq as u64) ||
        proof_off.iter().zip(proof_len).any(|(&o, &l)| o + l > proofs.len() as u64) ||
        content_off.iter().zip(count).any(|(&o, &c)| c > (1 << 53) || o + c * 1024 > content.len() as u64) {
        return Err(ChipError::InvalidArgument);
    }
    abi_audit()?;
    let mut lens = vec![0u64; nreq];
    check(unsafe {
        ffi_audit::chipa_verify_proofs_dev(proofs.as_ptr(), proof_off.as_ptr(), proof_len.as_ptr(),
                                           content_len.as_ptr(), hashes.as_ptr(), index.as_ptr(), count.as_ptr(),
                                           nreq as u64, content.as_mut_ptr(), content_off.as_ptr(), lens.as_mut_ptr(),
                                           status.as_mut_ptr() as *mut u32, scratch.ptr, stream.0)
    })?;
    Ok(lens)
}

/// scrub (decoding.rs:151-212) of every row: one result per stream
/// (Ok = repaired into that row of `out`; UnnecessaryScrub = intact).
/// Synchronous.
#[allow(clippy::too_many_arguments)]
pub fn scrub_batch(input: &DeviceRows, len: u64, hashes: &DeviceBuffer, padding: u32, chunk_len: u32,
                   out: &mut DeviceRows, scratch: &mut DeviceBuffer, stream: Stream) -> Result<Vec<Result<()>>> {
    input.holds(input.count, len)?;
    out.holds(input.count, len)?;
    if hashes.len() < input.count as usize * HASH_LEN ||
        (scratch.len() as u64) < unsafe { ffi::chip_scrub_scratch_len(len, input.count) } {
        return Err(ChipError::InvalidArgument);
    }
    let mut status = vec![0i32; input.count as usize];
    check(unsafe {
        ffi::chip_scrub_batch_dev(input.as_ptr(), input.stride, len, input.count, hashes.as_ptr(), padding, chunk_len,
                                  out.as_mut_ptr(), out.stride, status.as_mut_ptr(), scratch.ptr, stream.0)
    })?;
    Ok(status.into_iter().map(check).collect())
}

fn abi_repair() -> Result<()> {
    abi()?;
    match unsafe { ffi_repair::chipr_abi_version() } {
        ffi_repair::CHIPR_ABI_VERSION => Ok(()),
        v => Err(ChipError::AbiMismatch(v)),
    }
}

/// Scratch of a [`scrub_ragged`] / [`shard_masks_ragged`] call over streams of
/// these lengths that repairs any `nrepair` of them per pass (`in_len.len()`:
/// one pass; 1: the least a call accepts).
pub fn scrub_ragged_scratch_len(in_len: &[u64], nrepair: u64) -> u64 {
    unsafe { ffi_repair::chipr_scrub_ragged_scratch_len(in_len.as_ptr(), in_len.len() as u64, nrepair) }
}

/// The authentic zfec shards of every resident Bao|Zfec stream (stream o =
/// `input[in_off[o]..][..in_len[o]]`, `hashes[32 o..]` its hash, `chunk_len[o]`
/// its EncodeInfo's): `masks` (u32 per stream, on the device) gets bit i set
/// when shard i verifies; 0xFF = intact.  Enqueued on `stream`, not
/// synchronised.
#[allow(clippy::too_many_arguments)]
pub fn shard_masks_ragged(input: &DeviceBuffer, in_off: &[u64], in_len: &[u64], hashes: &DeviceBuffer,
                          chunk_len: &[u32], masks: &mut DeviceBuffer, scratch: &mut DeviceBuffer, stream: Stream)
                          -> Result<()> {
    let count = in_len.len();
    if in_off.len() != count || chunk_len.len() != count || hashes.len() < count * HASH_LEN ||
        masks.len() < count * 4 || in_off.iter().zip(in_len).any(|(&o, &l)| o + l > input.len() as u64) {
        return Err(ChipError::InvalidArgument);
    }
    abi_repair()?;
    check(unsafe {
        ffi_repair::chipr_shard_masks_ragged_dev(input.as_ptr(), in_off.as_ptr(), in_len.as_ptr(), count as u64,
                                                 hashes.as_ptr(), chunk_len.as_ptr(), masks.as_mut_ptr() as *mut u32,
                                                 scratch.ptr, scratch.len() as u64, stream.0)
    })
}

/// scrub (decoding.rs:151-212) of resident Bao|Zfec streams of different
/// lengths in one call: one result per stream (Ok = repaired into
/// `out[out_off[o]..][..in_len[o]]`; UnnecessaryScrub = intact; an output
/// range is written only for Ok).  The repairs run in as many passes as
/// `scratch` requires ([`scrub_ragged_scratch_len`]).  Synchronous.  (In place
/// repair, where output and input ranges coincide, needs the raw call: here
/// `out` is borrowed apart from `input`.)
#[allow(clippy::too_many_arguments)]
pub fn scrub_ragged(input: &DeviceBuffer, in_off: &[u64], in_len: &[u64], hashes: &DeviceBuffer, padding: &[u32],
                    chunk_len: &[u32], out: &mut DeviceBuffer, out_off: &[u64], scratch: &mut DeviceBuffer,
                    stream: Stream) -> Result<Vec<Result<()>>> {
    let count = in_len.len();
    if in_off.len() != count || padding.len() != count || chunk_len.len() != count || out_off.len() != count ||
        hashes.len() < count * HASH_LEN || in_off.iter().zip(in_len).any(|(&o, &l)| o + l > input.len() as u64) ||
        out_off.iter().zip(in_len).any(|(&o, &l)| o + l > out.len() as u64) {
        return Err(ChipError::InvalidArgument);
    }
    abi_repair()?;
    let mut status = vec![0i32; count];
    check(unsafe {
        ffi_repair::chipr_scrub_ragged_dev(input.as_ptr(), in_off.as_ptr(), in_len.as_ptr(), count as u64,
                                           hashes.as_ptr(), padding.as_ptr(), chunk_len.as_ptr(), out.as_mut_ptr(),
                                           out_off.as_ptr(), status.as_mut_ptr(), scratch.ptr, scratch.len() as u64,
                                           stream.0)
    })?;
    Ok(status.into_iter().map(check).collect())
}

fn abi_read() -> Result<()> {
    abi()?;
    match unsafe { ffi_read::chipd_abi_version() } {
        ffi_read::CHIPD_ABI_VERSION => Ok(()),
        v => Err(ChipError::AbiMismatch(v)),
    }
}

/// Where a [`read_ranges`] caller puts every request's content (host only):
/// (content_off, content_len, content_total, nseg), every range on a multiple
/// of `align` (a multiple of 16); `nseg` is for [`read_scratch_len`].
pub fn read_layout(chunk_len: &[u32], padding: &[u32], req_stream: &[u32], start: &[u64], len: &[u64], align: u64)
                   -> Result<(Vec<u64>, Vec<u64>, u64, u64)> {
    let nreq = req_stream.len();
    if padding.len() != chunk_len.len() || start.len() != nreq || len.len() != nreq {
        return Err(ChipError::InvalidArgument);
    }
    let (mut off, mut clen, mut total, mut nseg) = (vec![0u64; nreq], vec![0u64; nreq], 0u64, 0u64);
    check(unsafe {
        ffi_read::chipd_read_layout(chunk_len.as_ptr(), padding.as_ptr(), chunk_len.len() as u64, req_stream.as_ptr(),
                                    start.as_ptr(), len.as_ptr(), nreq as u64, align, off.as_mut_ptr(),
                                    clen.as_mut_ptr(), &mut total, &mut nseg)
    })?;
    Ok((off, clen, total, nseg))
}

/// Scratch of a [`read_ranges`] call of `nreq` requests in `nseg` segments.
pub fn read_scratch_len(nreq: u64, nseg: u64) -> u64 {
    unsafe { ffi_read::chipd_read_scratch_len(nreq, nseg) }
}

/// Object bytes `[start[r], start[r] + len[r])` of resident Zfec|Bao stream
/// `req_stream[r]` (stream s = `input[in_off[s]..][..in_len[s]]`) into
/// `content[content_off[r]..]`: copied where the primary's chunks verify,
/// rebuilt from four other authentic shards where they do not.  `status` and
/// `used` (u32 per request, on the device) get 0 or 7 and the shards each
/// request was served from.  Enqueued on `stream`, not synchronised.  Returns
/// the content length per request.
#[allow(clippy::too_many_arguments)]
pub fn read_ranges(input: &DeviceBuffer, in_off: &[u64], in_len: &[u64], hashes: &DeviceBuffer, padding: &[u32],
                   chunk_len: &[u32], req_stream: &[u32], start: &[u64], len: &[u64], content: &mut DeviceBuffer,
                   content_off: &[u64], status: &mut DeviceBuffer, used: &mut DeviceBuffer, scratch: &mut DeviceBuffer,
                   stream: Stream) -> Result<Vec<u64>> {
    let (count, nreq) = (in_len.len(), req_stream.len());
    if in_off.len() != count || padding.len() != count || chunk_len.len() != count || start.len() != nreq ||
        len.len() != nreq || content_off.len() != nreq || hashes.len() < count * HASH_LEN ||
        status.len() < nreq * 4 || used.len() < nreq * 4 ||
        in_off.iter().zip(in_len).any(|(&o, &l)| o + l > input.len() as u64) {
        return Err(ChipError::InvalidArgument);
    }
    let (_, want, _, _) = read_layout(chunk_len, padding, req_stream, start, len, 16)?;
    if content_off.iter().zip(&want).any(|(&o, &l)| o + l > content.len() as u64) {
        return Err(ChipError::InvalidArgument);
    }
    abi_read()?;
    let mut clen = vec![0u64; nreq];
    check(unsafe {
        ffi_read::chipd_read_ranges_dev(input.as_ptr(), in_off.as_ptr(), in_len.as_ptr(), hashes.as_ptr(),
                                        padding.as_ptr(), chunk_len.as_ptr(), count as u64, req_stream.as_ptr(),
                                        start.as_ptr(), len.as_ptr(), nreq as u64, content.as_mut_ptr(),
                                        content_off.as_ptr(), clen.as_mut_ptr(), status.as_mut_ptr() as *mut u32,
                                        used.as_mut_ptr() as *mut u32, scratch.ptr, scratch.len() as u64, stream.0)
    })?;
    Ok(clen)
}

fn abi_vread() -> Result<()> {
    abi_read()?;
    match unsafe { ffi_vread::chipv_abi_version() } {
        ffi_vread::CHIPV_ABI_VERSION => Ok(()),
        v => Err(ChipError::AbiMismatch(v)),
    }
}

/// Bits of a request's vouch word ([`read_ranges_vouched`]).
pub const VOUCHED: u32 = ffi_vread::CHIPV_VOUCHED;
pub const UNVOUCHED: u32 = ffi_vread::CHIPV_UNVOUCHED;
pub const CONTRADICTED: u32 = ffi_vread::CHIPV_CONTRADICTED;
/// Flag of [`read_ranges_vouched`]: a request with an unvouched segment fails with 7.
pub const VREAD_STRICT: u32 = ffi_vread::CHIPV_STRICT;

/// Scratch of a [`read_ranges_vouched`] call of `nreq` requests in `nseg`
/// segments ([`read_layout`]).
pub fn vread_scratch_len(nreq: u64, nseg: u64) -> u64 {
    unsafe { ffi_vread::chipv_read_scratch_len(nreq, nseg) }
}

/// [`read_ranges`] with every rebuilt chunk hashed against the CV the stream's
/// own tree stores for it.  `vouch` (u32 per request, on the device) gets the
/// OR over the request's segments of [`VOUCHED`], [`UNVOUCHED`] (the path to
/// the root is damaged too: rebuilt bytes with `read_ranges`' guarantee) and
/// [`CONTRADICTED`] (the rebuilt chunk does not hash to its stored CV: status
/// 5, zeros).  With status 0 and no [`UNVOUCHED`] bit every byte handed out is
/// hashed against the root; with [`VREAD_STRICT`] in `flags` status 0 alone
/// says so.  Enqueued on `stream`, not synchronised.  Returns the content
/// length per request.
#[allow(clippy::too_many_arguments)]
pub fn read_ranges_vouched(input: &DeviceBuffer, in_off: &[u64], in_len: &[u64], hashes: &DeviceBuffer,
                           padding: &[u32], chunk_len: &[u32], req_stream: &[u32], start: &[u64], len: &[u64],
                           content: &mut DeviceBuffer, content_off: &[u64], status: &mut DeviceBuffer,
                           used: &mut DeviceBuffer, vouch: &mut DeviceBuffer, flags: u32, scratch: &mut DeviceBuffer,
                           stream: Stream) -> Result<Vec<u64>> {
    let (count, nreq) = (in_len.len(), req_stream.len());
    if in_off.len() != count || padding.len() != count || chunk_len.len() != count || start.len() != nreq ||
        len.len() != nreq || content_off.len() != nreq || hashes.len() < count * HASH_LEN ||
        status.len() < nreq * 4 || used.len() < nreq * 4 || vouch.len() < nreq * 4 ||
        in_off.iter().zip(in_len).any(|(&o, &l)| o + l > input.len() as u64) {
        return Err(ChipError::InvalidArgument);
    }
    let (_, want, _, _) = read_layout(chunk_len, padding, req_stream, start, len, 16)?;
    if content_off.iter().zip(&want).any(|(&o, &l)| o + l > content.len() as u64) {
        return Err(ChipError::InvalidArgument);
    }
    abi_vread()?;
    let mut clen = vec![0u64; nreq];
    check(unsafe {
        ffi_vread::chipv_read_ranges_dev(input.as_ptr(), in_off.as_ptr(), in_len.as_ptr(), hashes.as_ptr(),
                                         padding.as_ptr(), chunk_len.as_ptr(), count as u64, req_stream.as_ptr(),
                                         start.as_ptr(), len.as_ptr(), nreq as u64, content.as_mut_ptr(),
                                         content_off.as_ptr(), clen.as_mut_ptr(), status.as_mut_ptr() as *mut u32,
                                         used.as_mut_ptr() as *mut u32, vouch.as_mut_ptr() as *mut u32, flags,
                                         scratch.ptr, scratch.len() as u64, stream.0)
    })?;
    Ok(clen)
}

fn abi_ecies() -> Result<()> {
    abi()?;
    match unsafe { ffi_ecies::chipe_abi_version() } {
        ffi_ecies::CHIPE_ABI_VERSION => Ok(()),
        v => Err(ChipError::AbiMismatch(v)),
    }
}

/// Status of a message whose tag does not verify ([`gcm_open_ragged`], [`ecies_open_ragged`]).
pub const ECIES_FAILED: u32 = 17;

/// Scratch of an AES-256-GCM call over messages of `n[o]` bytes.
pub fn gcm_scratch_len(n: &[u64]) -> u64 {
    unsafe { ffi_ecies::chipe_gcm_scratch_len(n.as_ptr(), n.len() as u64) }
}

fn ranges_fit(off: &[u64], len: &[u64], extra: u64, cap: usize) -> bool {
    off.iter().zip(len).all(|(&o, &l)| o.checked_add(l + extra).map_or(false, |e| e <= cap as u64))
}

/// AES-256-GCM (16-byte nonce, no AAD) of message o = `input[in_off[o]..][..n[o]]`
/// (16-B aligned) under `keys[32 o..]` and `ivs[16 o..]`: the ciphertext to
/// `out[out_off[o]..]` at any byte offset, the tag to `tags[16 o..]`.  A
/// bitsliced AES and a table-free GHASH on the device, constant time in keys
/// and plaintext; the key region of the scratch is zeroed by the call's last
/// operation.  Enqueued on `stream`, not synchronised.
#[allow(clippy::too_many_arguments)]
pub fn gcm_seal_ragged(keys: &[u8], ivs: &[u8], input: &DeviceBuffer, in_off: &[u64], n: &[u64],
                       out: &mut DeviceBuffer, out_off: &[u64], tags: &mut DeviceBuffer, scratch: &mut DeviceBuffer,
                       stream: Stream) -> Result<()> {
    let count = n.len();
    if keys.len() != 32 * count || ivs.len() != 16 * count || in_off.len() != count || out_off.len() != count ||
        tags.len() < 16 * count || !ranges_fit(in_off, n, 0, input.len()) || !ranges_fit(out_off, n, 0, out.len()) {
        return Err(ChipError::InvalidArgument);
    }
    abi_ecies()?;
    check(unsafe {
        ffi_ecies::chipe_gcm_seal_ragged_dev(keys.as_ptr(), ivs.as_ptr(), input.as_ptr(), in_off.as_ptr(), n.as_ptr(),
                                             count as u64, out.as_mut_ptr(), out_off.as_ptr(), tags.as_mut_ptr(),
                                             scratch.ptr, scratch.len() as u64, stream.0)
    })
}

/// The reverse of [`gcm_seal_ragged`]: the tags are checked first and the CTR
/// pass is gated on the verdicts on the device, so a message whose tag fails
/// gets `status[o]` = [`ECIES_FAILED`] (u32 per message, on the device) and
/// zeros over its whole range, the others 0 and their plaintext at
/// `out[out_off[o]..]` (16-B aligned).  Enqueued on `stream`, not synchronised.
#[allow(clippy::too_many_arguments)]
pub fn gcm_open_ragged(keys: &[u8], ivs: &[u8], input: &DeviceBuffer, in_off: &[u64], n: &[u64], tags: &DeviceBuffer,
                       out: &mut DeviceBuffer, out_off: &[u64], status: &mut DeviceBuffer, scratch: &mut DeviceBuffer,
                       stream: Stream) -> Result<()> {
    let count = n.len();
    if keys.len() != 32 * count || ivs.len() != 16 * count || in_off.len() != count || out_off.len() != count ||
        tags.len() < 16 * count || status.len() < 4 * count || !ranges_fit(in_off, n, 0, input.len()) ||
        !ranges_fit(out_off, n, 0, out.len()) {
        return Err(ChipError::InvalidArgument);
    }
    abi_ecies()?;
    check(unsafe {
        ffi_ecies::chipe_gcm_open_ragged_dev(keys.as_ptr(), ivs.as_ptr(), input.as_ptr(), in_off.as_ptr(), n.as_ptr(),
                                             count as u64, tags.as_ptr(), out.as_mut_ptr(), out_off.as_ptr(),
                                             status.as_mut_ptr() as *mut u32, scratch.ptr, scratch.len() as u64,
                                             stream.0)
    })
}

/// `encoding::ecies` of every resident object to the receiver `pubkey`: the
/// envelope eph_pub65 || nonce16 || tag16 || ciphertext, `n[o] + 97` bytes, to
/// `out[out_off[o]..]`.  The key agreement of every object runs on the host
/// before anything is enqueued; `scratch` holds [`gcm_scratch_len`]`(n)` bytes.
/// Enqueued on `stream`, not synchronised.
#[allow(clippy::too_many_arguments)]
pub fn ecies_seal_ragged(pubkey: &[u8], input: &DeviceBuffer, in_off: &[u64], n: &[u64], out: &mut DeviceBuffer,
                         out_off: &[u64], scratch: &mut DeviceBuffer, stream: Stream) -> Result<()> {
    let count = n.len();
    if in_off.len() != count || out_off.len() != count || !ranges_fit(in_off, n, 0, input.len()) ||
        !ranges_fit(out_off, n, 97, out.len()) || (scratch.len() as u64) < gcm_scratch_len(n) {
        return Err(ChipError::InvalidArgument);
    }
    abi_ecies()?;
    check(unsafe {
        ffi_ecies::chipe_seal_ragged_dev(pubkey.as_ptr(), pubkey.len() as u64, ptr::null(), input.as_ptr(),
                                         in_off.as_ptr(), n.as_ptr(), count as u64, out.as_mut_ptr(), out_off.as_ptr(),
                                         scratch.ptr, stream.0)
    })
}

/// `decoding::ecies` of every resident envelope `input[in_off[o]..][..in_len[o]]`:
/// the plaintext to `out[out_off[o]..]` (16-B aligned) and `status[o]` = 0, or
/// [`ECIES_FAILED`] and zeros.  The call waits once, for the envelopes' header
/// bytes (the keys depend on them).  Returns the plaintext length per object.
#[allow(clippy::too_many_arguments)]
pub fn ecies_open_ragged(secret_key: &[u8], input: &DeviceBuffer, in_off: &[u64], in_len: &[u64],
                         out: &mut DeviceBuffer, out_off: &[u64], status: &mut DeviceBuffer,
                         scratch: &mut DeviceBuffer, stream: Stream) -> Result<Vec<u64>> {
    let count = in_len.len();
    let plain: Vec<u64> = in_len.iter().map(|&l| l.saturating_sub(97)).collect();
    if in_off.len() != count || out_off.len() != count || status.len() < 4 * count ||
        !ranges_fit(in_off, in_len, 0, input.len()) || !ranges_fit(out_off, &plain, 0, out.len()) ||
        (scratch.len() as u64) < gcm_scratch_len(&plain) {
        return Err(ChipError::InvalidArgument);
    }
    abi_ecies()?;
    let mut olen = vec![0u64; count];
    check(unsafe {
        ffi_ecies::chipe_open_ragged_dev(secret_key.as_ptr(), secret_key.len() as u64, input.as_ptr(), in_off.as_ptr(),
                                         in_len.as_ptr(), count as u64, out.as_mut_ptr(), out_off.as_ptr(),
                                         olen.as_mut_ptr(), status.as_mut_ptr() as *mut u32, scratch.ptr, stream.0)
    })?;
    Ok(olen)
}

/// Scratch of [`encode_ragged_ecies`] (object lengths) / [`decode_ragged_ecies`] (stream lengths).
pub fn ecies_ragged_scratch_len(format: u8, lens: &[u64], decode: bool) -> u64 {
    unsafe {
        if decode {
            ffi_ecies::chipe_decode_scratch_len(format, lens.as_ptr(), lens.len() as u64)
        } else {
            ffi_ecies::chipe_encode_scratch_len(format, lens.as_ptr(), lens.len() as u64)
        }
    }
}

/// encode() at Ecies with Bao and / or Zfec (5, 9, 13) of resident objects in
/// one call: sealed into envelopes in the scratch, then encoded as
/// [`encode_ragged`] does at `format & 12` (offsets: [`ragged_layout`] of the
/// sizes + 97).  Stream bytes, hash and `EncodeInfo` are those of [`encode`].
#[allow(clippy::too_many_arguments)]
pub fn encode_ragged_ecies(format: u8, pubkey: &[u8], input: &DeviceBuffer, in_off: &[u64], sizes: &[u64],
                           out: &mut DeviceBuffer, out_off: &[u64], hashes: &mut DeviceBuffer,
                           scratch: &mut DeviceBuffer, stream: Stream) -> Result<(Vec<u64>, Vec<ChipEncodeInfo>)> {
    let count = sizes.len();
    let env: Vec<u64> = sizes.iter().map(|&n| n + 97).collect();
    let need_scratch = ecies_ragged_scratch_len(format, sizes, false);
    if in_off.len() != count || out_off.len() != count || hashes.len() < count * HASH_LEN || need_scratch == 0 ||
        (scratch.len() as u64) < need_scratch || !ranges_fit(in_off, sizes, 0, input.len()) {
        return Err(ChipError::InvalidArgument);
    }
    let (_, need, _) = ragged_layout(format & 12, &env, 256, 0)?;
    if !ranges_fit(out_off, &need, 0, out.len()) {
        return Err(ChipError::InvalidArgument);
    }
    abi_ecies()?;
    let mut lens = vec![0u64; count];
    let mut infos = vec![ChipEncodeInfo::default(); count];
    check(unsafe {
        ffi_ecies::chipe_encode_ragged_dev(format, pubkey.as_ptr(), pubkey.len() as u64, ptr::null(), input.as_ptr(),
                                           in_off.as_ptr(), sizes.as_ptr(), count as u64, out.as_mut_ptr(),
                                           out_off.as_ptr(), lens.as_mut_ptr(), hashes.as_mut_ptr(), infos.as_mut_ptr(),
                                           scratch.ptr, stream.0)
    })?;
    Ok((lens, infos))
}

/// decode() at 5, 9 or 13 of resident streams in one call: [`decode_ragged`] at
/// `format & 12` into envelopes in the scratch, then [`ecies_open_ragged`]
/// (which waits once).  `status[o]`: 0, the bao status of a damaged stream (not
/// opened, zeros) or [`ECIES_FAILED`].  `out` must hold `in_len[o]` bytes from
/// `out_off[o]`.  Returns the plaintext lengths.
#[allow(clippy::too_many_arguments)]
pub fn decode_ragged_ecies(format: u8, secret_key: &[u8], input: &DeviceBuffer, in_off: &[u64], in_len: &[u64],
                           hashes: &DeviceBuffer, padding: &[u32], out: &mut DeviceBuffer, out_off: &[u64],
                           status: &mut DeviceBuffer, scratch: &mut DeviceBuffer, stream: Stream) -> Result<Vec<u64>> {
    let count = in_len.len();
    let need_scratch = ecies_ragged_scratch_len(format, in_len, true);
    if in_off.len() != count || out_off.len() != count || padding.len() != count || hashes.len() < count * HASH_LEN ||
        status.len() < 4 * count || need_scratch == 0 || (scratch.len() as u64) < need_scratch ||
        !ranges_fit(in_off, in_len, 0, input.len()) || !ranges_fit(out_off, in_len, 0, out.len()) {
        return Err(ChipError::InvalidArgument);
    }
    abi_ecies()?;
    let mut olen = vec![0u64; count];
    check(unsafe {
        ffi_ecies::chipe_decode_ragged_dev(format, secret_key.as_ptr(), secret_key.len() as u64, input.as_ptr(),
                                           in_off.as_ptr(), in_len.as_ptr(), count as u64, hashes.as_ptr(),
                                           padding.as_ptr(), out.as_mut_ptr(), out_off.as_ptr(), olen.as_mut_ptr(),
                                           status.as_mut_ptr() as *mut u32, scratch.ptr, stream.0)
    })?;
    Ok(olen)
}

fn abi_snap() -> Result<()> {
    abi()?;
    match unsafe { ffi_snap::chips_abi_version() } {
        ffi_snap::CHIPS_ABI_VERSION => Ok(()),
        v => Err(ChipError::AbiMismatch(v)),
    }
}

/// Status of a stream that is no valid frame stream ([`unsnap_ragged`], [`decode_ragged_snap`]).
pub const SNAP_FAILED: u32 = 16;

/// Scratch of [`snap_ragged`] over objects of `n[o]` bytes (`out_cap` = None),
/// or of [`unsnap_ragged`] over streams of `n[o]` bytes into these capacities.
pub fn snap_scratch(n: &[u64], out_cap: Option<&[u64]>) -> u64 {
    unsafe {
        match out_cap {
            None => ffi_snap::chips_snap_scratch_len(n.as_ptr(), n.len() as u64),
            Some(cap) if cap.len() == n.len() => {
                ffi_snap::chips_unsnap_scratch_len(n.as_ptr(), cap.as_ptr(), n.len() as u64)
            }
            Some(_) => 0,
        }
    }
}

/// `encoding::snap` of every resident object `input[in_off[o]..][..n[o]]`
/// (16-B aligned): its frame stream, bit-exact with [`snap_compress`], to
/// `out[out_off[o]..]` at any byte offset (capacity `chip_snap_max_len(n[o])`),
/// its length to `out_len[o]` (u64 per object, on the device).  Enqueued on
/// `stream`, not synchronised.
#[allow(clippy::too_many_arguments)]
pub fn snap_ragged(input: &DeviceBuffer, in_off: &[u64], n: &[u64], out: &mut DeviceBuffer, out_off: &[u64],
                   out_len: &mut DeviceBuffer, scratch: &mut DeviceBuffer, stream: Stream) -> Result<()> {
    let count = n.len();
    let worst: Vec<u64> = n.iter().map(|&x| unsafe { ffi::chip_snap_max_len(x) }).collect();
    if in_off.len() != count || out_off.len() != count || out_len.len() < 8 * count ||
        !ranges_fit(in_off, n, 0, input.len()) || !ranges_fit(out_off, &worst, 0, out.len()) {
        return Err(ChipError::InvalidArgument);
    }
    abi_snap()?;
    check(unsafe {
        ffi_snap::chips_snap_ragged_dev(input.as_ptr(), in_off.as_ptr(), n.as_ptr(), count as u64, out.as_mut_ptr(),
                                        out_off.as_ptr(), out_len.as_mut_ptr() as *mut u64, scratch.ptr,
                                        scratch.len() as u64, stream.0)
    })
}

/// `decoding::snap` of every resident frame stream `input[in_off[o]..][..in_len[o]]`
/// (any byte offset) into `out[out_off[o]..]` (16-B aligned, capacity
/// `out_cap[o]`): `status[o]` (u32) and `out_len[o]` (u64), both on the device,
/// are what [`snap_decompress`] gives.  A stream that fails leaves no
/// decompressed byte.  Enqueued on `stream`, not synchronised.
#[allow(clippy::too_many_arguments)]
pub fn unsnap_ragged(input: &DeviceBuffer, in_off: &[u64], in_len: &[u64], out: &mut DeviceBuffer, out_off: &[u64],
                     out_cap: &[u64], out_len: &mut DeviceBuffer, status: &mut DeviceBuffer,
                     scratch: &mut DeviceBuffer, stream: Stream) -> Result<()> {
    let count = in_len.len();
    if in_off.len() != count || out_off.len() != count || out_cap.len() != count || out_len.len() < 8 * count ||
        status.len() < 4 * count || !ranges_fit(in_off, in_len, 0, input.len()) ||
        !ranges_fit(out_off, out_cap, 0, out.len()) {
        return Err(ChipError::InvalidArgument);
    }
    abi_snap()?;
    check(unsafe {
        ffi_snap::chips_unsnap_ragged_dev(input.as_ptr(), in_off.as_ptr(), in_len.as_ptr(), count as u64,
                                          out.as_mut_ptr(), out_off.as_ptr(), out_cap.as_ptr(),
                                          out_len.as_mut_ptr() as *mut u64, status.as_mut_ptr() as *mut u32,
                                          scratch.ptr, scratch.len() as u64, stream.0)
    })
}

/// Where [`encode_ragged_snap`]'s caller should put each object: [`ragged_layout`]
/// over the worst-case lengths, since the encoded length depends on the data.
/// Returns (out_off, out_cap, total).
pub fn snap_encode_layout(format: u8, sizes: &[u64], align: u64, stream_offset: u64)
                          -> Result<(Vec<u64>, Vec<u64>, u64)> {
    let mut off = vec![0u64; sizes.len()];
    let mut cap = vec![0u64; sizes.len()];
    let mut total = 0u64;
    check(unsafe {
        ffi_snap::chips_encode_layout(format, sizes.as_ptr(), sizes.len() as u64, align, stream_offset,
                                      off.as_mut_ptr(), cap.as_mut_ptr(), &mut total)
    })?;
    Ok((off, cap, total))
}

/// Scratch of [`encode_ragged_snap`] (object lengths, `out_cap` = None) or of
/// [`decode_ragged_snap`] (stream lengths and output capacities).
pub fn snap_ragged_scratch(format: u8, lens: &[u64], out_cap: Option<&[u64]>) -> u64 {
    unsafe {
        match out_cap {
            None => ffi_snap::chips_encode_scratch_len(format, lens.as_ptr(), lens.len() as u64),
            Some(cap) if cap.len() == lens.len() => {
                ffi_snap::chips_decode_scratch_len(format, lens.as_ptr(), cap.as_ptr(), lens.len() as u64)
            }
            Some(_) => 0,
        }
    }
}

/// encode() at a format with the Snappy bit and Bao and / or Zfec (6, 7, 10,
/// 11, 14, 15) of resident objects in one call: compressed into rows of the
/// scratch, then (sealed to `pubkey` with the Ecies bit and) encoded as
/// [`encode_ragged`] does at `format & 12` (offsets: [`snap_encode_layout`]).
/// The call waits once, for the compressed lengths.  Stream bytes, hash and
/// `EncodeInfo` are those of [`encode`].
#[allow(clippy::too_many_arguments)]
pub fn encode_ragged_snap(format: u8, pubkey: &[u8], input: &DeviceBuffer, in_off: &[u64], sizes: &[u64],
                          out: &mut DeviceBuffer, out_off: &[u64], hashes: &mut DeviceBuffer,
                          scratch: &mut DeviceBuffer, stream: Stream) -> Result<(Vec<u64>, Vec<ChipEncodeInfo>)> {
    let count = sizes.len();
    let need_scratch = snap_ragged_scratch(format, sizes, None);
    if in_off.len() != count || out_off.len() != count || hashes.len() < count * HASH_LEN || need_scratch == 0 ||
        (scratch.len() as u64) < need_scratch || !ranges_fit(in_off, sizes, 0, input.len()) {
        return Err(ChipError::InvalidArgument);
    }
    let (_, cap, _) = snap_encode_layout(format, sizes, 256, 0)?;
    if !ranges_fit(out_off, &cap, 0, out.len()) {
        return Err(ChipError::InvalidArgument);
    }
    abi_snap()?;
    let mut lens = vec![0u64; count];
    let mut infos = vec![ChipEncodeInfo::default(); count];
    let pk = if pubkey.is_empty() { ptr::null() } else { pubkey.as_ptr() };
    check(unsafe {
        ffi_snap::chips_encode_ragged_dev(format, pk, pubkey.len() as u64, ptr::null(), input.as_ptr(),
                                          in_off.as_ptr(), sizes.as_ptr(), count as u64, out.as_mut_ptr(),
                                          out_off.as_ptr(), lens.as_mut_ptr(), hashes.as_mut_ptr(), infos.as_mut_ptr(),
                                          scratch.ptr, stream.0)
    })?;
    Ok((lens, infos))
}

/// decode() at 6, 7, 10, 11, 14 or 15 of resident streams in one call:
/// [`decode_ragged`] (or [`decode_ragged_ecies`]) into rows of the scratch, then
/// [`unsnap_ragged`] into `out[out_off[o]..]` (capacity `out_cap[o]`).
/// `status[o]` (u32, on the device): 0, the bao / ecies status of an object
/// that failed there (not decompressed, nothing written) or a snappy status;
/// `out_len[o]` (u64, on the device): the decoded length.  Without the Ecies
/// bit nothing is waited for.
#[allow(clippy::too_many_arguments)]
pub fn decode_ragged_snap(format: u8, secret_key: &[u8], input: &DeviceBuffer, in_off: &[u64], in_len: &[u64],
                          hashes: &DeviceBuffer, padding: &[u32], out: &mut DeviceBuffer, out_off: &[u64],
                          out_cap: &[u64], out_len: &mut DeviceBuffer, status: &mut DeviceBuffer,
                          scratch: &mut DeviceBuffer, stream: Stream) -> Result<()> {
    let count = in_len.len();
    let need_scratch = snap_ragged_scratch(format, in_len, Some(out_cap));
    if in_off.len() != count || out_off.len() != count || out_cap.len() != count || padding.len() != count ||
        hashes.len() < count * HASH_LEN || status.len() < 4 * count || out_len.len() < 8 * count ||
        need_scratch == 0 || (scratch.len() as u64) < need_scratch || !ranges_fit(in_off, in_len, 0, input.len()) ||
        !ranges_fit(out_off, out_cap, 0, out.len()) {
        return Err(ChipError::InvalidArgument);
    }
    abi_snap()?;
    let sk = if secret_key.is_empty() { ptr::null() } else { secret_key.as_ptr() };
    check(unsafe {
        ffi_snap::chips_decode_ragged_dev(format, sk, secret_key.len() as u64, input.as_ptr(), in_off.as_ptr(),
                                          in_len.as_ptr(), count as u64, hashes.as_ptr(), padding.as_ptr(),
                                          out.as_mut_ptr(), out_off.as_ptr(), out_cap.as_ptr(),
                                          out_len.as_mut_ptr() as *mut u64, status.as_mut_ptr() as *mut u32,
                                          scratch.ptr, stream.0)
    })
}

/// encode() of `count` objects in HOST memory, H2D / kernels / D2H and the
/// host stages overlapped over `nslots` device slots.  Returns the encoded
/// length of every object; streams at `out[o * out_stride..]`, hashes at
/// `hashes[32 o..]`.  At Zfec|Bao the library writes each stream's header and
/// data-shard chunks from the host and copies only the rest back; with a host
/// stage and `out` in pinned memory it also reads the device's input from
/// `out` (the call holds `&mut out` for its whole duration, so that is safe).
#[allow(clippy::too_many_arguments)]
pub fn encode_host_batch(format: u8, pubkey: &[u8], input: &[u8], n: usize, count: usize, in_stride: usize,
                         out: &mut [u8], out_stride: usize, hashes: &mut [u8], infos: Option<&mut [ChipEncodeInfo]>,
                         nslots: u32, slice_bytes: u64, host_threads: u32) -> Result<Vec<u64>> {
    let in_need = if count == 0 { 0 } else { (count - 1) * in_stride + n };
    if input.len() < in_need || out_stride < encode_max_len(n) || out.len() < count * out_stride ||
        hashes.len() < count * HASH_LEN ||
        infos.as_ref().map_or(false, |i| i.len() < count) {
        return Err(ChipError::InvalidArgument);
    }
    abi()?;
    let mut lens = vec![0u64; count];
    check(unsafe {
        ffi::chip_encode_host_batch(format, pubkey.as_ptr(), pubkey.len() as u64, ptr::null(), input.as_ptr(), n as u64,
                                    count as u64, in_stride as u64, out.as_mut_ptr(), out_stride as u64,
                                    lens.as_mut_ptr(), hashes.as_mut_ptr(),
                                    infos.map_or(ptr::null_mut(), |i| i.as_mut_ptr()), nslots, slice_bytes,
                                    host_threads)
    })?;
    Ok(lens)
}

/// decode() of `count` encodings in HOST memory; one result per object
/// (a corrupted object does not fail its neighbours).
#[allow(clippy::too_many_arguments)]
pub fn decode_host_batch(format: u8, secret_key: &[u8], hashes: &[u8], input: &[u8], in_len: &[u64],
                         in_stride: usize, padding: &[u32], out: &mut [u8], out_stride: usize, nslots: u32,
                         slice_bytes: u64, host_threads: u32) -> Result<Vec<Result<u64>>> {
    let count = in_len.len();
    if padding.len() < count || hashes.len() < count * HASH_LEN || out.len() < count * out_stride ||
        in_len.iter().enumerate().any(|(o, &l)| o * in_stride + l as usize > input.len()) {
        return Err(ChipError::InvalidArgument);
    }
    abi()?;
    let mut lens = vec![0u64; count];
    let mut status = vec![0i32; count];
    let rc = unsafe {
        ffi::chip_decode_host_batch(format, secret_key.as_ptr(), secret_key.len() as u64, hashes.as_ptr(),
                                    input.as_ptr(), in_len.as_ptr(), count as u64, in_stride as u64, padding.as_ptr(),
                                    out.as_mut_ptr(), out_stride as u64, lens.as_mut_ptr(), status.as_mut_ptr(),
                                    nslots, slice_bytes, host_threads)
    };
    if rc != ffi::CHIP_OK && status.iter().all(|&s| s == ffi::CHIP_OK) {
        return Err(ChipError::from_status(rc, 0, 0)); // a call-level failure, not an object's
    }
    Ok(status
        .into_iter()
        .zip(lens)
        .map(|(s, l)| if s == ffi::CHIP_OK { Ok(l) } else { Err(ChipError::from_status(s, HASH_LEN, l)) })
        .collect())
}

fn abi_cread() -> Result<()> {
    abi_vread()?;
    abi_ecies()?;
    match unsafe { ffi_cread::chipc_abi_version() } {
        ffi_cread::CHIPC_ABI_VERSION => Ok(()),
        v => Err(ChipError::AbiMismatch(v)),
    }
}

/// Scratch of a [`ctr_ranges`] call over `nitems` items under `nkeys` keys.
pub fn ctr_scratch(nkeys: u64, nitems: u64) -> u64 {
    unsafe { ffi_cread::chipc_ctr_scratch_len(nkeys, nitems) }
}

/// Item i XORs `buf[buf_off[i]..][..n[i]]` (16-B aligned) in place with
/// keystream bytes `[pos[i], pos[i] + n[i])` of AES-256-GCM (16-byte nonce)
/// under `keys[32 k..]` and `ivs[16 k..]`, k = `item_key[i]`.  The same call
/// encrypts and decrypts.  `gate`: u32 per item on the device; item i is
/// skipped where its word is not zero.  Constant time in keys and keystream;
/// the key region of the scratch is zeroed by the call's last operation.
/// Enqueued on `stream`, not synchronised.
#[allow(clippy::too_many_arguments)]
pub fn ctr_ranges(keys: &[u8], ivs: &[u8], item_key: &[u32], pos: &[u64], n: &[u64], buf: &mut DeviceBuffer,
                  buf_off: &[u64], gate: Option<&DeviceBuffer>, scratch: &mut DeviceBuffer, stream: Stream)
                  -> Result<()> {
    let (nkeys, nitems) = (keys.len() / 32, n.len());
    if keys.len() != 32 * nkeys || ivs.len() != 16 * nkeys || item_key.len() != nitems || pos.len() != nitems ||
        buf_off.len() != nitems || !ranges_fit(buf_off, n, 0, buf.len()) ||
        gate.map_or(false, |g| g.len() < 4 * nitems) {
        return Err(ChipError::InvalidArgument);
    }
    abi_cread()?;
    check(unsafe {
        ffi_cread::chipc_ctr_ranges_dev(keys.as_ptr(), ivs.as_ptr(), nkeys as u64, item_key.as_ptr(), pos.as_ptr(),
                                        n.as_ptr(), nitems as u64, buf.as_mut_ptr(), buf_off.as_ptr(),
                                        gate.map_or(std::ptr::null(), |g| g.as_ptr() as *const u32), scratch.ptr,
                                        scratch.len() as u64, stream.0)
    })
}

/// Scratch of a [`stream_keys`] call over `nstreams` streams.
pub fn stream_keys_scratch(nstreams: u64) -> u64 {
    unsafe { ffi_cread::chipc_stream_keys_scratch_len(nstreams) }
}

/// The AES key and nonce of every resident level-13 stream: envelope bytes
/// `[0, 81)` read by a strict vouched read (so only bytes hashed against the
/// root), one key agreement per stream on the host.  The call waits once, for
/// the header bytes.  Returns (keys, 32 bytes per stream; nonces, 16 bytes per
/// stream; key status per stream: 0, 5 or 7 for a header that cannot be served,
/// 17 for an object shorter than 97 bytes or an ephemeral key that does not
/// parse, with zeros for key and nonce).  The keys are the caller's to wipe.
#[allow(clippy::too_many_arguments)]
pub fn stream_keys(secret_key: &[u8], input: &DeviceBuffer, in_off: &[u64], in_len: &[u64], hashes: &DeviceBuffer,
                   padding: &[u32], chunk_len: &[u32], scratch: &mut DeviceBuffer, stream: Stream)
                   -> Result<(Vec<u8>, Vec<u8>, Vec<u32>)> {
    let count = in_len.len();
    if in_off.len() != count || padding.len() != count || chunk_len.len() != count ||
        hashes.len() < count * HASH_LEN || !ranges_fit(in_off, in_len, 0, input.len()) {
        return Err(ChipError::InvalidArgument);
    }
    abi_cread()?;
    let (mut keys, mut ivs, mut status) = (vec![0u8; 32 * count], vec![0u8; 16 * count], vec![0u32; count]);
    check(unsafe {
        ffi_cread::chipc_stream_keys_dev(secret_key.as_ptr(), secret_key.len() as u64, input.as_ptr(), in_off.as_ptr(),
                                         in_len.as_ptr(), hashes.as_ptr(), padding.as_ptr(), chunk_len.as_ptr(),
                                         count as u64, keys.as_mut_ptr(), ivs.as_mut_ptr(), status.as_mut_ptr(),
                                         scratch.ptr, scratch.len() as u64, stream.0)
    })?;
    Ok((keys, ivs, status))
}

/// [`read_layout`] for requests in plaintext bytes of level-13 streams:
/// plaintext `[start, min(P, start + len))` with P = 4 chunk_len - padding - 97.
pub fn plain_read_layout(chunk_len: &[u32], padding: &[u32], req_stream: &[u32], start: &[u64], len: &[u64],
                         align: u64) -> Result<(Vec<u64>, Vec<u64>, u64, u64)> {
    let nreq = req_stream.len();
    if padding.len() != chunk_len.len() || start.len() != nreq || len.len() != nreq {
        return Err(ChipError::InvalidArgument);
    }
    let (mut off, mut clen, mut total, mut nseg) = (vec![0u64; nreq], vec![0u64; nreq], 0u64, 0u64);
    check(unsafe {
        ffi_cread::chipc_read_layout(chunk_len.as_ptr(), padding.as_ptr(), chunk_len.len() as u64,
                                     req_stream.as_ptr(), start.as_ptr(), len.as_ptr(), nreq as u64, align,
                                     off.as_mut_ptr(), clen.as_mut_ptr(), &mut total, &mut nseg)
    })?;
    Ok((off, clen, total, nseg))
}

/// Scratch of a [`read_plain_ranges`] call of `nreq` requests in `nseg`
/// segments ([`plain_read_layout`]) over `nstreams` streams.
pub fn plain_read_scratch(nreq: u64, nseg: u64, nstreams: u64) -> u64 {
    unsafe { ffi_cread::chipc_read_scratch_len(nreq, nseg, nstreams) }
}

/// Plaintext bytes `[start[r], start[r] + len[r])` of resident level-13 stream
/// `req_stream[r]` into `content[content_off[r]..]`, with `keys`, `ivs` and
/// `key_status` as [`stream_keys`] gave them: [`read_ranges_vouched`] of the
/// envelope bytes behind the range, then the keystream taken off in place,
/// gated on the read's status.  A request whose stream has a non-zero key
/// status gets that status, zeros, used 0 and vouch 0.  The GCM tag is NOT
/// checked: the ciphertext is vouched for by the root hash, and a wrong key
/// gives status 0 and bytes that are not the plaintext.  Enqueued on `stream`,
/// not synchronised.  Returns the content length per request.
#[allow(clippy::too_many_arguments)]
pub fn read_plain_ranges(keys: &[u8], ivs: &[u8], key_status: Option<&[u32]>, input: &DeviceBuffer, in_off: &[u64],
                         in_len: &[u64], hashes: &DeviceBuffer, padding: &[u32], chunk_len: &[u32],
                         req_stream: &[u32], start: &[u64], len: &[u64], content: &mut DeviceBuffer,
                         content_off: &[u64], status: &mut DeviceBuffer, used: &mut DeviceBuffer,
                         vouch: &mut DeviceBuffer, flags: u32, scratch: &mut DeviceBuffer, stream: Stream)
                         -> Result<Vec<u64>> {
    let (count, nreq) = (in_len.len(), req_stream.len());
    if keys.len() != 32 * count || ivs.len() != 16 * count || key_status.map_or(false, |k| k.len() != count) ||
        in_off.len() != count || padding.len() != count || chunk_len.len() != count || start.len() != nreq ||
        len.len() != nreq || content_off.len() != nreq || hashes.len() < count * HASH_LEN ||
        status.len() < nreq * 4 || used.len() < nreq * 4 || vouch.len() < nreq * 4 ||
        !ranges_fit(in_off, in_len, 0, input.len()) {
        return Err(ChipError::InvalidArgument);
    }
    let (_, want, _, _) = plain_read_layout(chunk_len, padding, req_stream, start, len, 16)?;
    if !ranges_fit(content_off, &want, 0, content.len()) {
        return Err(ChipError::InvalidArgument);
    }
    abi_cread()?;
    let mut clen = vec![0u64; nreq];
    check(unsafe {
        ffi_cread::chipc_read_ranges_dev(keys.as_ptr(), ivs.as_ptr(), key_status.map_or(std::ptr::null(), |k| k.as_ptr()),
                                         input.as_ptr(), in_off.as_ptr(), in_len.as_ptr(), hashes.as_ptr(),
                                         padding.as_ptr(), chunk_len.as_ptr(), count as u64, req_stream.as_ptr(),
                                         start.as_ptr(), len.as_ptr(), nreq as u64, content.as_mut_ptr(),
                                         content_off.as_ptr(), clen.as_mut_ptr(), status.as_mut_ptr() as *mut u32,
                                         used.as_mut_ptr() as *mut u32, vouch.as_mut_ptr() as *mut u32, flags,
                                         scratch.ptr, scratch.len() as u64, stream.0)
    })?;
    Ok(clen)
}

fn abi_fread() -> Result<()> {
    abi_cread()?;
    match unsafe { ffi_fread::chipf_abi_version() } {
        ffi_fread::CHIPF_ABI_VERSION => Ok(()),
        v => Err(ChipError::AbiMismatch(v)),
    }
}

/// The frame index of resident level-14 / level-15 streams: `nframes[s] + 1`
/// ascending offsets into stream s's frame stream from entry `idx_off[s]` of
/// `frame_off`, the last one its length; with what proved it.
#[derive(Debug, Clone, Default)]
pub struct FrameIndex {
    pub frame_off: Vec<u64>,
    pub idx_off: Vec<u64>,
    pub nframes: Vec<u64>,
    /// 0 for a proven index; 2 for a capacity below `nframes + 1`; 11 for a valid
    /// stream that is not canonical; 5, 7 or 16 (with a vouch bit where a header's
    /// primary copy is damaged: scrub, then build again); the stream's key status.
    pub index_status: Vec<u32>,
    pub plain_len: Vec<u64>,
    pub index_vouch: Vec<u32>,
}

fn key_ptrs(format: u8, keys: Option<(&[u8], &[u8])>, key_status: Option<&[u32]>, count: usize)
            -> Result<(*const u8, *const u8, *const u32)> {
    match (format, keys) {
        (15, Some((k, v))) if k.len() == 32 * count && v.len() == 16 * count &&
            key_status.map_or(true, |s| s.len() == count) =>
            Ok((k.as_ptr(), v.as_ptr(), key_status.map_or(ptr::null(), |s| s.as_ptr()))),
        (14, _) => Ok((ptr::null(), ptr::null(), ptr::null())),
        _ => Err(ChipError::InvalidArgument),
    }
}

/// Scratch of a [`frame_index`] or [`verify_frame_index`] call over `nstreams`
/// streams and `nentries` index entries in all.
pub fn frame_index_scratch(nstreams: u64, nentries: u64) -> u64 {
    unsafe { ffi_fread::chipf_index_scratch_len(nstreams, nentries) }
}

/// Builds and proves the frame index of every resident level-14 / level-15
/// stream (`keys`: the AES keys and nonces of [`stream_keys`], for format 15):
/// a serial walk over the chunk headers of the primary copy, then
/// [`verify_frame_index`]'s work over what it found.  Stream s may write
/// `idx_cap[s]` entries from entry `idx_off[s]`.  The call waits twice.
#[allow(clippy::too_many_arguments)]
pub fn frame_index(format: u8, keys: Option<(&[u8], &[u8])>, key_status: Option<&[u32]>, input: &DeviceBuffer,
                   in_off: &[u64], in_len: &[u64], hashes: &DeviceBuffer, padding: &[u32], chunk_len: &[u32],
                   idx_off: &[u64], idx_cap: &[u64], scratch: &mut DeviceBuffer, stream: Stream)
                   -> Result<FrameIndex> {
    let count = in_len.len();
    if in_off.len() != count || padding.len() != count || chunk_len.len() != count || idx_off.len() != count ||
        idx_cap.len() != count || hashes.len() < count * HASH_LEN || !ranges_fit(in_off, in_len, 0, input.len()) {
        return Err(ChipError::InvalidArgument);
    }
    let (pk, pv, pks) = key_ptrs(format, keys, key_status, count)?;
    abi_fread()?;
    let total = idx_off.iter().zip(idx_cap).map(|(o, c)| o.saturating_add(*c)).max().unwrap_or(0);
    let mut ix = FrameIndex {
        frame_off: vec![0u64; total as usize],
        idx_off: idx_off.to_vec(),
        nframes: vec![0u64; count],
        index_status: vec![0u32; count],
        plain_len: vec![0u64; count],
        index_vouch: vec![0u32; count],
    };
    check(unsafe {
        ffi_fread::chipf_frame_index_dev(format, pk, pv, pks, input.as_ptr(), in_off.as_ptr(), in_len.as_ptr(),
                                         hashes.as_ptr(), padding.as_ptr(), chunk_len.as_ptr(), count as u64,
                                         ix.frame_off.as_mut_ptr(), idx_off.as_ptr(), idx_cap.as_ptr(),
                                         ix.nframes.as_mut_ptr(), ix.index_status.as_mut_ptr(),
                                         ix.plain_len.as_mut_ptr(), ix.index_vouch.as_mut_ptr(), scratch.ptr,
                                         scratch.len() as u64, stream.0)
    })?;
    Ok(ix)
}

/// Proves `index` against the streams: a strict vouched read of the identifier
/// and of every chunk header, the keystream over them at 15, the chain check.
/// `index_status` (u32), `plain_len` (u64) and `index_vouch` (u32), one entry
/// per stream on the device.  Enqueued on `stream`, not synchronised.
#[allow(clippy::too_many_arguments)]
pub fn verify_frame_index(format: u8, keys: Option<(&[u8], &[u8])>, key_status: Option<&[u32]>, input: &DeviceBuffer,
                          in_off: &[u64], in_len: &[u64], hashes: &DeviceBuffer, padding: &[u32], chunk_len: &[u32],
                          index: &FrameIndex, index_status: &mut DeviceBuffer, plain_len: &mut DeviceBuffer,
                          index_vouch: &mut DeviceBuffer, scratch: &mut DeviceBuffer, stream: Stream) -> Result<()> {
    let count = in_len.len();
    if in_off.len() != count || padding.len() != count || chunk_len.len() != count || !index_holds(index, count) ||
        hashes.len() < count * HASH_LEN || index_status.len() < 4 * count || plain_len.len() < 8 * count ||
        index_vouch.len() < 4 * count || !ranges_fit(in_off, in_len, 0, input.len()) {
        return Err(ChipError::InvalidArgument);
    }
    let (pk, pv, pks) = key_ptrs(format, keys, key_status, count)?;
    abi_fread()?;
    check(unsafe {
        ffi_fread::chipf_verify_index_dev(format, pk, pv, pks, input.as_ptr(), in_off.as_ptr(), in_len.as_ptr(),
                                          hashes.as_ptr(), padding.as_ptr(), chunk_len.as_ptr(), count as u64,
                                          index.frame_off.as_ptr(), index.idx_off.as_ptr(), index.nframes.as_ptr(),
                                          index_status.as_mut_ptr() as *mut u32, plain_len.as_mut_ptr() as *mut u64,
                                          index_vouch.as_mut_ptr() as *mut u32, scratch.ptr, scratch.len() as u64,
                                          stream.0)
    })
}

// every stream's entries lie inside the index's offsets
fn index_holds(index: &FrameIndex, count: usize) -> bool {
    index.idx_off.len() == count && index.nframes.len() == count && index.plain_len.len() == count &&
        index.idx_off.iter().zip(&index.nframes).all(|(o, n)| {
            o.checked_add(*n).and_then(|e| e.checked_add(1)).map_or(false, |e| e <= index.frame_off.len() as u64)
        })
}

/// What [`read_frame_ranges`] needs of the requests: content offsets and lengths
/// of plaintext `[start, min(plain_len, start + len))`, their total, the number
/// of (request, frame) work items, the bytes of the staging rows and the
/// segments of the vouched read.
#[derive(Debug, Clone, Default)]
pub struct FrameReadLayout {
    pub content_off: Vec<u64>,
    pub content_len: Vec<u64>,
    pub content_total: u64,
    pub nseg: u64,
    pub stage_total: u64,
    pub vseg: u64,
}

/// Host only: the layout of the requests over `index` (with its `index_status`
/// as the read takes it).
#[allow(clippy::too_many_arguments)]
pub fn frame_read_layout(format: u8, chunk_len: &[u32], padding: &[u32], index: &FrameIndex, use_status: bool,
                         req_stream: &[u32], start: &[u64], len: &[u64], align: u64) -> Result<FrameReadLayout> {
    let (count, nreq) = (chunk_len.len(), req_stream.len());
    if padding.len() != count || !index_holds(index, count) || start.len() != nreq || len.len() != nreq ||
        (use_status && index.index_status.len() != count) {
        return Err(ChipError::InvalidArgument);
    }
    let mut l = FrameReadLayout { content_off: vec![0u64; nreq], content_len: vec![0u64; nreq], ..Default::default() };
    check(unsafe {
        ffi_fread::chipf_read_layout(format, chunk_len.as_ptr(), padding.as_ptr(),
                                     if use_status { index.index_status.as_ptr() } else { ptr::null() },
                                     index.frame_off.as_ptr(), index.idx_off.as_ptr(), index.nframes.as_ptr(),
                                     index.plain_len.as_ptr(), count as u64, req_stream.as_ptr(), start.as_ptr(),
                                     len.as_ptr(), nreq as u64, align, l.content_off.as_mut_ptr(),
                                     l.content_len.as_mut_ptr(), &mut l.content_total, &mut l.nseg,
                                     &mut l.stage_total, &mut l.vseg)
    })?;
    Ok(l)
}

/// Scratch of a [`read_frame_ranges`] call (the numbers of [`frame_read_layout`]).
pub fn frame_read_scratch(layout: &FrameReadLayout, nstreams: u64) -> u64 {
    unsafe {
        ffi_fread::chipf_read_scratch_len(layout.content_off.len() as u64, layout.nseg, layout.stage_total, layout.vseg,
                                          nstreams)
    }
}

/// Plaintext bytes `[start[r], start[r] + len[r])` of resident level-14 /
/// level-15 stream `req_stream[r]` into `content[content_off[r]..]` (any byte
/// offset), with an index that [`frame_index`] or [`verify_frame_index`]
/// proved: [`read_ranges_vouched`] of the compressed frames behind the range,
/// the keystream taken off them at 15, one block decode per frame with header
/// and CRC checked, only the wanted bytes stored.  Status per request: 0, the
/// read's 5 or 7, 16 for a frame that disagrees with the index or its CRC (a
/// wrong key at 15 among them), or the stream's index status where `use_status`
/// and that is not zero; content is the exact plaintext for 0, zeros otherwise.
/// The GCM tag is NOT checked.  Enqueued on `stream`, not synchronised.  Returns
/// the content length per request.
#[allow(clippy::too_many_arguments)]
pub fn read_frame_ranges(format: u8, keys: Option<(&[u8], &[u8])>, index: &FrameIndex, use_status: bool,
                         input: &DeviceBuffer, in_off: &[u64], in_len: &[u64], hashes: &DeviceBuffer, padding: &[u32],
                         chunk_len: &[u32], req_stream: &[u32], start: &[u64], len: &[u64],
                         content: &mut DeviceBuffer, content_off: &[u64], status: &mut DeviceBuffer,
                         used: &mut DeviceBuffer, vouch: &mut DeviceBuffer, flags: u32, scratch: &mut DeviceBuffer,
                         stream: Stream) -> Result<Vec<u64>> {
    let (count, nreq) = (in_len.len(), req_stream.len());
    if in_off.len() != count || padding.len() != count || chunk_len.len() != count || content_off.len() != nreq ||
        hashes.len() < count * HASH_LEN || status.len() < nreq * 4 || used.len() < nreq * 4 || vouch.len() < nreq * 4 ||
        !ranges_fit(in_off, in_len, 0, input.len()) {
        return Err(ChipError::InvalidArgument);
    }
    let want = frame_read_layout(format, chunk_len, padding, index, use_status, req_stream, start, len, 16)?;
    if !ranges_fit(content_off, &want.content_len, 0, content.len()) {
        return Err(ChipError::InvalidArgument);
    }
    let (pk, pv, _) = key_ptrs(format, keys, None, count)?;
    abi_fread()?;
    let mut clen = vec![0u64; nreq];
    check(unsafe {
        ffi_fread::chipf_read_ranges_dev(format, pk, pv,
                                         if use_status { index.index_status.as_ptr() } else { ptr::null() },
                                         index.frame_off.as_ptr(), index.idx_off.as_ptr(), index.nframes.as_ptr(),
                                         index.plain_len.as_ptr(), input.as_ptr(), in_off.as_ptr(), in_len.as_ptr(),
                                         hashes.as_ptr(), padding.as_ptr(), chunk_len.as_ptr(), count as u64,
                                         req_stream.as_ptr(), start.as_ptr(), len.as_ptr(), nreq as u64,
                                         content.as_mut_ptr(), content_off.as_ptr(), clen.as_mut_ptr(),
                                         status.as_mut_ptr() as *mut u32, used.as_mut_ptr() as *mut u32,
                                         vouch.as_mut_ptr() as *mut u32, flags, scratch.ptr, scratch.len() as u64,
                                         stream.0)
    })?;
    Ok(clen)
}

fn abi_qread() -> Result<()> {
    abi_vread()?;
    match unsafe { ffi_qread::chipq_abi_version() } {
        ffi_qread::CHIPQ_ABI_VERSION => Ok(()),
        v => Err(ChipError::AbiMismatch(v)),
    }
}

/// What the planned reads know of a stream table: the number of streams, the
/// largest chunk count and the smallest non-zero shard length among them.
pub type TableInfo = ffi_qread::chipq_table_info;

/// Bytes of device memory the table of `nstreams` streams needs ([`stream_table`]).
pub fn stream_table_len(nstreams: u64) -> u64 {
    unsafe { ffi_qread::chipq_stream_table_len(nstreams) }
}

/// Describe resident streams once (the stream arguments of [`read_ranges`])
/// in `table`, for every later [`read_ranges_planned`] call.  The one upload,
/// enqueued on `stream`; the table stays valid while the streams and hashes
/// stay where they are.
#[allow(clippy::too_many_arguments)]
pub fn stream_table(input: &DeviceBuffer, in_off: &[u64], in_len: &[u64], hashes: &DeviceBuffer, padding: &[u32],
                    chunk_len: &[u32], table: &mut DeviceBuffer, stream: Stream) -> Result<TableInfo> {
    let count = in_len.len();
    if in_off.len() != count || padding.len() != count || chunk_len.len() != count ||
        hashes.len() < count * HASH_LEN || (table.len() as u64) < stream_table_len(count as u64) ||
        !ranges_fit(in_off, in_len, 0, input.len()) {
        return Err(ChipError::InvalidArgument);
    }
    abi_qread()?;
    let mut info = TableInfo::default();
    check(unsafe {
        ffi_qread::chipq_stream_table_dev(input.as_ptr(), in_off.as_ptr(), in_len.as_ptr(), hashes.as_ptr(),
                                          padding.as_ptr(), chunk_len.as_ptr(), count as u64, table.ptr,
                                          table.len() as u64, &mut info, stream.0)
    })?;
    Ok(info)
}

/// Scratch of a [`read_ranges_planned`] (`vouched`: [`read_ranges_vouched_planned`])
/// call of capacity (`nreq`, `max_len`); 0 where the call would refuse it.
pub fn planned_read_scratch_len(info: &TableInfo, nreq: u64, max_len: u64, vouched: bool) -> u64 {
    unsafe { ffi_qread::chipq_read_scratch_len(info, nreq, max_len, vouched as u32) }
}

fn planned_fits(nreq: u64, max_len: u64, req_stream: &DeviceBuffer, start: &DeviceBuffer, len: &DeviceBuffer,
                content: &DeviceBuffer, content_stride: u64, content_len: &DeviceBuffer, words: &[&DeviceBuffer])
                -> bool {
    let n = nreq as usize;
    let slot = (max_len + 15) / 16 * 16;
    req_stream.len() >= n * 4 && start.len() >= n * 8 && len.len() >= n * 8 && content_len.len() >= n * 8 &&
        words.iter().all(|w| w.len() >= n * 4) &&
        (nreq == 0 || (nreq - 1).checked_mul(content_stride).and_then(|x| x.checked_add(slot.min(content_stride)))
            .map_or(false, |e| e <= content.len() as u64))
}

/// [`read_ranges`] for requests that live on the device: `req_stream` (u32),
/// `start` and `len` (u64) are device arrays of `nreq` entries, read by the
/// GPU only; `nreq` and `max_len` are the capacity of the call (spare
/// requests: length 0).  Request r's content goes to
/// `content[r * content_stride..]`, its length to `content_len[r]` (u64, on
/// the device).  The host work is O(1) and nothing is uploaded.  Enqueued on
/// `stream`, not synchronised.
#[allow(clippy::too_many_arguments)]
pub fn read_ranges_planned(table: &DeviceBuffer, info: &TableInfo, req_stream: &DeviceBuffer, start: &DeviceBuffer,
                           len: &DeviceBuffer, nreq: u64, max_len: u64, content: &mut DeviceBuffer,
                           content_stride: u64, content_len: &mut DeviceBuffer, status: &mut DeviceBuffer,
                           used: &mut DeviceBuffer, scratch: &mut DeviceBuffer, stream: Stream) -> Result<()> {
    if !planned_fits(nreq, max_len, req_stream, start, len, content, content_stride, content_len, &[status, used]) {
        return Err(ChipError::InvalidArgument);
    }
    abi_qread()?;
    check(unsafe {
        ffi_qread::chipq_read_ranges_dev(table.ptr, info, req_stream.as_ptr() as *const u32,
                                         start.as_ptr() as *const u64, len.as_ptr() as *const u64, nreq, max_len,
                                         content.as_mut_ptr(), content_stride, content_len.as_mut_ptr() as *mut u64,
                                         status.as_mut_ptr() as *mut u32, used.as_mut_ptr() as *mut u32, scratch.ptr,
                                         scratch.len() as u64, stream.0)
    })
}

/// [`read_ranges_vouched`] for requests that live on the device: the
/// arguments of [`read_ranges_planned`], the vouch word per request and
/// `flags` (0 or [`VREAD_STRICT`]) as there.
#[allow(clippy::too_many_arguments)]
pub fn read_ranges_vouched_planned(table: &DeviceBuffer, info: &TableInfo, req_stream: &DeviceBuffer,
                                   start: &DeviceBuffer, len: &DeviceBuffer, nreq: u64, max_len: u64,
                                   content: &mut DeviceBuffer, content_stride: u64, content_len: &mut DeviceBuffer,
                                   status: &mut DeviceBuffer, used: &mut DeviceBuffer, vouch: &mut DeviceBuffer,
                                   flags: u32, scratch: &mut DeviceBuffer, stream: Stream) -> Result<()> {
    if !planned_fits(nreq, max_len, req_stream, start, len, content, content_stride, content_len,
                     &[status, used, vouch]) {
        return Err(ChipError::InvalidArgument);
    }
    abi_qread()?;
    check(unsafe {
        ffi_qread::chipq_read_ranges_vouched_dev(table.ptr, info, req_stream.as_ptr() as *const u32,
                                                 start.as_ptr() as *const u64, len.as_ptr() as *const u64, nreq,
                                                 max_len, content.as_mut_ptr(), content_stride,
                                                 content_len.as_mut_ptr() as *mut u64, status.as_mut_ptr() as *mut u32,
                                                 used.as_mut_ptr() as *mut u32, vouch.as_mut_ptr() as *mut u32, flags,
                                                 scratch.ptr, scratch.len() as u64, stream.0)
    })
}

fn abi_kread() -> Result<()> {
    abi_qread()?;
    abi_cread()?;
    match unsafe { ffi_kread::chipk_abi_version() } {
        ffi_kread::CHIPK_ABI_VERSION => Ok(()),
        v => Err(ChipError::AbiMismatch(v)),
    }
}

/// Bytes of device memory the key table of `nstreams` streams needs ([`key_table`]).
pub fn key_table_len(nstreams: u64) -> u64 {
    unsafe { ffi_kread::chipk_key_table_len(nstreams) }
}

/// Expand the keys of resident level-13 streams once (`keys`, `ivs` and
/// `key_status` as [`stream_keys`] gave them) into `table`, for every later
/// [`read_plain_ranges_planned`] call: round keys and J0 per stream, zeros for
/// a stream whose key status is not 0.  The raw keys pass through a staging
/// part of the table that is zeros again once the enqueued work is done; the
/// round keys STAY in `table` until [`wipe_key_table`].  Enqueued on `stream`.
pub fn key_table(keys: &[u8], ivs: &[u8], key_status: Option<&[u32]>, table: &mut DeviceBuffer, stream: Stream)
                 -> Result<()> {
    let count = keys.len() / 32;
    if keys.len() != 32 * count || ivs.len() != 16 * count || key_status.map_or(false, |k| k.len() != count) ||
        (table.len() as u64) < key_table_len(count as u64) {
        return Err(ChipError::InvalidArgument);
    }
    abi_kread()?;
    check(unsafe {
        ffi_kread::chipk_key_table_dev(keys.as_ptr(), ivs.as_ptr(), key_status.map_or(ptr::null(), |k| k.as_ptr()),
                                       count as u64, table.ptr, table.len() as u64, stream.0)
    })
}

/// Zeros over the whole key table, enqueued on `stream` behind the reads that use it.
pub fn wipe_key_table(table: &mut DeviceBuffer, stream: Stream) -> Result<()> {
    abi_kread()?;
    check(unsafe { ffi_kread::chipk_key_table_wipe_dev(table.ptr, table.len() as u64, stream.0) })
}

/// Scratch of a [`read_plain_ranges_planned`] call of capacity (`nreq`,
/// `max_len`); 0 where the call would refuse it.
pub fn planned_plain_read_scratch_len(info: &TableInfo, nreq: u64, max_len: u64) -> u64 {
    unsafe { ffi_kread::chipk_read_scratch_len(info, nreq, max_len) }
}

/// [`read_plain_ranges`] for requests that live on the device: the arguments
/// of [`read_ranges_vouched_planned`] with requests in PLAINTEXT bytes of
/// level-13 streams, over the stream table and the key table ([`key_table`])
/// of the same streams.  A request the device refuses has status 1; a request
/// on a stream whose key status is not 0 has that status, zeros over its
/// clipped range, used 0 and vouch 0.  Kernel launches only; enqueued on
/// `stream`, not synchronised.
#[allow(clippy::too_many_arguments)]
pub fn read_plain_ranges_planned(table: &DeviceBuffer, info: &TableInfo, key_table: &DeviceBuffer,
                                 req_stream: &DeviceBuffer, start: &DeviceBuffer, len: &DeviceBuffer, nreq: u64,
                                 max_len: u64, content: &mut DeviceBuffer, content_stride: u64,
                                 content_len: &mut DeviceBuffer, status: &mut DeviceBuffer, used: &mut DeviceBuffer,
                                 vouch: &mut DeviceBuffer, flags: u32, scratch: &mut DeviceBuffer, stream: Stream)
                                 -> Result<()> {
    if !planned_fits(nreq, max_len, req_stream, start, len, content, content_stride, content_len,
                     &[status, used, vouch]) {
        return Err(ChipError::InvalidArgument);
    }
    abi_kread()?;
    check(unsafe {
        ffi_kread::chipk_read_ranges_dev(table.ptr, info, key_table.ptr, key_table.len() as u64,
                                         req_stream.as_ptr() as *const u32, start.as_ptr() as *const u64,
                                         len.as_ptr() as *const u64, nreq, max_len, content.as_mut_ptr(),
                                         content_stride, content_len.as_mut_ptr() as *mut u64,
                                         status.as_mut_ptr() as *mut u32, used.as_mut_ptr() as *mut u32,
                                         vouch.as_mut_ptr() as *mut u32, flags, scratch.ptr, scratch.len() as u64,
                                         stream.0)
    })
}

fn abi_gread() -> Result<()> {
    abi_kread()?;
    abi_fread()?;
    match unsafe { ffi_gread::chipg_abi_version() } {
        ffi_gread::CHIPG_ABI_VERSION => Ok(()),
        v => Err(ChipError::AbiMismatch(v)),
    }
}

/// What the planned reads know of a frame table: the number of streams, the
/// index entries it holds, the longest frame among them and the format (14 or
/// 15).
pub type FrameInfo = ffi_gread::chipg_frame_info;

/// Bytes of device memory the frame table of `nstreams` streams with
/// `nentries` index entries in all needs ([`frame_table`]).
pub fn frame_table_len(nstreams: u64, nentries: u64) -> u64 {
    unsafe { ffi_gread::chipg_frame_table_len(nstreams, nentries) }
}

/// Describe the frame indexes of resident level-14 / level-15 streams once
/// (the index arguments of [`read_frame_ranges`], as [`frame_index`] or
/// [`verify_frame_index`] proved them) in `table`, for every later
/// [`read_frame_ranges_planned`] call: the checks that call makes of every
/// index on every call, made once, and the one upload, enqueued on `stream`.
/// The table stays valid while the streams are not re-encoded.
#[allow(clippy::too_many_arguments)]
pub fn frame_table(format: u8, chunk_len: &[u32], padding: &[u32], index_status: Option<&[u32]>, frame_off: &[u64],
                   idx_off: &[u64], nframes: &[u64], plain_len: &[u64], table: &mut DeviceBuffer, stream: Stream)
                   -> Result<FrameInfo> {
    let count = chunk_len.len();
    if padding.len() != count || idx_off.len() != count || nframes.len() != count || plain_len.len() != count ||
        index_status.map_or(false, |k| k.len() != count) ||
        idx_off.iter().zip(nframes).any(|(&o, &n)| {
            o.checked_add(n).and_then(|e| e.checked_add(1)).map_or(true, |e| e > frame_off.len() as u64)
        }) {
        return Err(ChipError::InvalidArgument);
    }
    abi_gread()?;
    let mut info = FrameInfo::default();
    check(unsafe {
        ffi_gread::chipg_frame_table_dev(format, chunk_len.as_ptr(), padding.as_ptr(),
                                         index_status.map_or(ptr::null(), |k| k.as_ptr()), frame_off.as_ptr(),
                                         idx_off.as_ptr(), nframes.as_ptr(), plain_len.as_ptr(), count as u64,
                                         table.ptr, table.len() as u64, &mut info, stream.0)
    })?;
    Ok(info)
}

/// Scratch of a [`read_frame_ranges_planned`] call of capacity (`nreq`,
/// `max_len`); 0 where the call would refuse it.
pub fn planned_frame_read_scratch_len(info: &TableInfo, finfo: &FrameInfo, nreq: u64, max_len: u64) -> u64 {
    unsafe { ffi_gread::chipg_read_scratch_len(info, finfo, nreq, max_len) }
}

/// [`read_frame_ranges`] for requests that live on the device: the arguments
/// of [`read_ranges_vouched_planned`] with requests in PLAINTEXT bytes of
/// level-14 / level-15 streams, over the stream table, the frame table
/// ([`frame_table`]) and, at 15, the key table ([`key_table`]; `None` at 14)
/// of the same streams.  A request the device refuses has status 1; a request
/// on a stream whose index status or key status is not 0 has that status,
/// zeros over its clipped range, used 0 and vouch 0.  Kernel launches only;
/// enqueued on `stream`, not synchronised.
#[allow(clippy::too_many_arguments)]
pub fn read_frame_ranges_planned(table: &DeviceBuffer, info: &TableInfo, frame_table: &DeviceBuffer,
                                 finfo: &FrameInfo, key_table: Option<&DeviceBuffer>, req_stream: &DeviceBuffer,
                                 start: &DeviceBuffer, len: &DeviceBuffer, nreq: u64, max_len: u64,
                                 content: &mut DeviceBuffer, content_stride: u64, content_len: &mut DeviceBuffer,
                                 status: &mut DeviceBuffer, used: &mut DeviceBuffer, vouch: &mut DeviceBuffer,
                                 flags: u32, scratch: &mut DeviceBuffer, stream: Stream) -> Result<()> {
    if !planned_fits(nreq, max_len, req_stream, start, len, content, content_stride, content_len,
                     &[status, used, vouch]) ||
        (frame_table.len() as u64) < frame_table_len(finfo.nstreams, finfo.nentries) {
        return Err(ChipError::InvalidArgument);
    }
    abi_gread()?;
    check(unsafe {
        ffi_gread::chipg_read_ranges_dev(table.ptr, info, frame_table.ptr, finfo,
                                         key_table.map_or(ptr::null(), |k| k.ptr as *const _),
                                         key_table.map_or(0, |k| k.len() as u64),
                                         req_stream.as_ptr() as *const u32, start.as_ptr() as *const u64,
                                         len.as_ptr() as *const u64, nreq, max_len, content.as_mut_ptr(),
                                         content_stride, content_len.as_mut_ptr() as *mut u64,
                                         status.as_mut_ptr() as *mut u32, used.as_mut_ptr() as *mut u32,
                                         vouch.as_mut_ptr() as *mut u32, flags, scratch.ptr, scratch.len() as u64,
                                         stream.0)
    })
}

fn abi_paudit() -> Result<()> {
    abi_qread()?;
    match unsafe { ffi_paudit::chipp_abi_version() } {
        ffi_paudit::CHIPP_ABI_VERSION => Ok(()),
        v => Err(ChipError::AbiMismatch(v)),
    }
}

/// What [`verify_slice_proofs_planned`] knows of a root table: the number of
/// audited streams and the largest chunk count among them.
pub type RootInfo = ffi_paudit::chipp_root_info;

/// `req_stream` of a spare slot of a planned audit.
pub const NO_REQUEST: u32 = ffi_paudit::CHIPP_NO_REQUEST;

/// Bytes of device memory the root table of `nroots` audited streams needs ([`root_table`]).
pub fn root_table_len(nroots: u64) -> u64 {
    unsafe { ffi_paudit::chipp_root_table_len(nroots) }
}

/// The auditor's one upload: stream s has `content_len[s]` content bytes and
/// its expected root is `hashes[32 s..]` (device, stays where it is).
/// Enqueued on `stream`.
pub fn root_table(content_len: &[u64], hashes: &DeviceBuffer, table: &mut DeviceBuffer, stream: Stream)
                  -> Result<RootInfo> {
    let count = content_len.len();
    if hashes.len() < count * HASH_LEN || (table.len() as u64) < root_table_len(count as u64) {
        return Err(ChipError::InvalidArgument);
    }
    abi_paudit()?;
    let mut info = RootInfo::default();
    check(unsafe {
        ffi_paudit::chipp_root_table_dev(content_len.as_ptr(), hashes.as_ptr(), count as u64, table.ptr,
                                         table.len() as u64, &mut info, stream.0)
    })?;
    Ok(info)
}

/// Scratch of a planned audit of capacity (`nreq`, `max_count`) over a table
/// whose largest chunk count is `max_chunks`; 0 where the call would refuse it.
pub fn planned_audit_scratch_len(max_chunks: u64, nreq: u64, max_count: u64) -> u64 {
    unsafe { ffi_paudit::chipp_audit_scratch_len(max_chunks, nreq, max_count) }
}

/// The most bytes a proof of `max_count` chunks of a stream of `max_chunks` chunks can have.
pub fn proof_bound(max_chunks: u64, max_count: u64) -> u64 {
    unsafe { ffi_paudit::chipp_proof_bound(max_chunks, max_count) }
}

fn slots_fit(nreq: u64, stride: u64, least: u64, buf: &DeviceBuffer) -> bool {
    nreq == 0 || (nreq - 1).checked_mul(stride).and_then(|x| x.checked_add(least.min(stride)))
        .map_or(false, |e| e <= buf.len() as u64)
}

fn audit_requests_fit(nreq: u64, req_stream: &DeviceBuffer, index: &DeviceBuffer, count: &DeviceBuffer,
                      lens: &[&DeviceBuffer], status: &DeviceBuffer) -> bool {
    let n = nreq as usize;
    req_stream.len() >= n * 4 && index.len() >= n * 8 && count.len() >= n * 8 && status.len() >= n * 4 &&
        lens.iter().all(|l| l.len() >= n * 8)
}

/// [`verify_slices`] for requests that live on the device: `req_stream` (u32;
/// [`NO_REQUEST`]: a spare slot), `index` and `count` (u64) are device arrays
/// of `nreq` entries, read by the GPU only; `nreq` and `max_count` (selected
/// chunks per request) are the capacity of the call.  Request r's content goes
/// to `content[r * content_stride..]`, its length to `content_len[r]` (u64, on
/// the device).  A request the device refuses has status 1.  Kernel launches
/// only; enqueued on `stream`, not synchronised.
#[allow(clippy::too_many_arguments)]
pub fn verify_slices_planned(table: &DeviceBuffer, info: &TableInfo, req_stream: &DeviceBuffer, index: &DeviceBuffer,
                             count: &DeviceBuffer, nreq: u64, max_count: u64, content: &mut DeviceBuffer,
                             content_stride: u64, content_len: &mut DeviceBuffer, status: &mut DeviceBuffer,
                             scratch: &mut DeviceBuffer, stream: Stream) -> Result<()> {
    if !audit_requests_fit(nreq, req_stream, index, count, &[content_len], status) ||
        !slots_fit(nreq, content_stride, max_count.saturating_mul(1024), content) {
        return Err(ChipError::InvalidArgument);
    }
    abi_paudit()?;
    check(unsafe {
        ffi_paudit::chipp_verify_slices_dev(table.ptr, info, req_stream.as_ptr() as *const u32,
                                            index.as_ptr() as *const u64, count.as_ptr() as *const u64, nreq,
                                            max_count, content.as_mut_ptr(), content_stride,
                                            content_len.as_mut_ptr() as *mut u64, status.as_mut_ptr() as *mut u32,
                                            scratch.ptr, scratch.len() as u64, stream.0)
    })
}

/// [`extract_slices`] for requests that live on the device (as
/// [`verify_slices_planned`]): request r's proof goes to
/// `proofs[r * proof_stride..]`, its exact length to `proof_len[r]` (u64, on
/// the device); `proof_stride` is at least [`proof_bound`].  Status 0, or 1
/// for a request the device refuses.
#[allow(clippy::too_many_arguments)]
pub fn extract_slices_planned(table: &DeviceBuffer, info: &TableInfo, req_stream: &DeviceBuffer, index: &DeviceBuffer,
                              count: &DeviceBuffer, nreq: u64, max_count: u64, proofs: &mut DeviceBuffer,
                              proof_stride: u64, proof_len: &mut DeviceBuffer, status: &mut DeviceBuffer,
                              scratch: &mut DeviceBuffer, stream: Stream) -> Result<()> {
    if !audit_requests_fit(nreq, req_stream, index, count, &[proof_len], status) ||
        !slots_fit(nreq, proof_stride, proof_bound(info.max_chunks, max_count), proofs) {
        return Err(ChipError::InvalidArgument);
    }
    abi_paudit()?;
    check(unsafe {
        ffi_paudit::chipp_extract_slices_dev(table.ptr, info, req_stream.as_ptr() as *const u32,
                                             index.as_ptr() as *const u64, count.as_ptr() as *const u64, nreq,
                                             max_count, proofs.as_mut_ptr(), proof_stride,
                                             proof_len.as_mut_ptr() as *mut u64, status.as_mut_ptr() as *mut u32,
                                             scratch.ptr, scratch.len() as u64, stream.0)
    })
}

/// The auditor's side for requests and proofs that live on the device:
/// `req_stream[r]` names the audited stream of the root table whose proof
/// sits in `proofs[r * proof_stride..]`, `proof_len[r]` (u64, on the device,
/// read) the bytes that arrived.  Status 6 where that is not the proof's exact
/// length (content zeros), else as [`verify_slices_planned`].
#[allow(clippy::too_many_arguments)]
pub fn verify_slice_proofs_planned(roots: &DeviceBuffer, root_info: &RootInfo, req_stream: &DeviceBuffer,
                                   index: &DeviceBuffer, count: &DeviceBuffer, nreq: u64, max_count: u64,
                                   proofs: &DeviceBuffer, proof_stride: u64, proof_len: &DeviceBuffer,
                                   content: &mut DeviceBuffer, content_stride: u64, content_len: &mut DeviceBuffer,
                                   status: &mut DeviceBuffer, scratch: &mut DeviceBuffer, stream: Stream)
                                   -> Result<()> {
    if !audit_requests_fit(nreq, req_stream, index, count, &[proof_len, content_len], status) ||
        !slots_fit(nreq, proof_stride, proof_bound(root_info.max_chunks, max_count), proofs) ||
        !slots_fit(nreq, content_stride, max_count.saturating_mul(1024), content) {
        return Err(ChipError::InvalidArgument);
    }
    abi_paudit()?;
    check(unsafe {
        ffi_paudit::chipp_verify_proofs_dev(roots.ptr, root_info, req_stream.as_ptr() as *const u32,
                                            index.as_ptr() as *const u64, count.as_ptr() as *const u64, nreq,
                                            max_count, proofs.as_ptr(), proof_stride,
                                            proof_len.as_ptr() as *const u64, content.as_mut_ptr(), content_stride,
                                            content_len.as_mut_ptr() as *mut u64, status.as_mut_ptr() as *mut u32,
                                            scratch.ptr, scratch.len() as u64, stream.0)
    })
}

fn abi_agree() -> Result<()> {
    abi_ecies()?;
    match unsafe { ffi_agree::chipy_abi_version() } {
        ffi_agree::CHIPY_ABI_VERSION => Ok(()),
        v => Err(ChipError::AbiMismatch(v)),
    }
}

/// Scratch of a [`seal_keys`] / [`open_keys`] call over `count` objects.
pub fn agree_scratch_len(count: u64) -> u64 {
    unsafe { ffi_agree::chipy_keys_scratch_len(count) }
}

/// Scratch of [`ecies_seal_ragged_dev_keys`] / [`ecies_open_ragged_dev_keys`] over plaintexts of `n[o]` bytes.
pub fn envelope_scratch_len(n: &[u64]) -> u64 {
    unsafe { ffi_agree::chipy_envelope_scratch_len(n.as_ptr(), n.len() as u64) }
}

fn pitched(buf_len: usize, pitch: u64, width: u64, count: u64) -> bool {
    count == 0 || (pitch >= width && (count - 1).checked_mul(pitch).and_then(|x| x.checked_add(width))
        .map_or(false, |e| e <= buf_len as u64))
}

/// The Ecies key agreement of a seal on the device, per object o: the
/// ephemeral public key k_o G (0x04 || x || y) to `pubs[o * pub_pitch..][..65]`
/// and the AES key HKDF(E65 || (k_o P)65) to `keys[o * key_pitch..][..32]`, P
/// the receiver `pubkey` (33 or 65 bytes).  `eph_sk`: 32 bytes per object, or
/// `None` for secrets from the library's RNG.  secp256k1 and HKDF-SHA256 run
/// as kernels, constant time in the scalars; the AES keys stay in `keys`, which
/// the caller wipes.  Enqueued on `stream`, not synchronised.
#[allow(clippy::too_many_arguments)]
pub fn seal_keys(pubkey: &[u8], eph_sk: Option<&[u8]>, count: u64, pubs: &mut DeviceBuffer, pub_pitch: u64,
                 keys: &mut DeviceBuffer, key_pitch: u64, scratch: &mut DeviceBuffer, stream: Stream) -> Result<()> {
    if eph_sk.map_or(false, |s| s.len() as u64 != 32 * count) || !pitched(pubs.len(), pub_pitch, 65, count) ||
        !pitched(keys.len(), key_pitch, 32, count) || (scratch.len() as u64) < agree_scratch_len(count) {
        return Err(ChipError::InvalidArgument);
    }
    abi_agree()?;
    check(unsafe {
        ffi_agree::chipy_seal_keys_dev(pubkey.as_ptr(), pubkey.len() as u64, eph_sk.map_or(ptr::null(), |s| s.as_ptr()),
                                       count, pubs.as_mut_ptr(), pub_pitch, keys.as_mut_ptr(), key_pitch, scratch.ptr,
                                       scratch.len() as u64, stream.0)
    })
}

/// The key agreement of an open on the device, per object o: the AES key
/// HKDF(R65 || (sk R)65) of the ephemeral key R = `eph[o * eph_pitch..][..65]`
/// to `keys[o * key_pitch..][..32]` and `status[o]` = 0 (u32 per object, on
/// the device); or [`ECIES_FAILED`] and a key of zeros for an R that does not
/// parse.  The AES keys stay in `keys`, which the caller wipes.  Enqueued on
/// `stream`, not synchronised.
#[allow(clippy::too_many_arguments)]
pub fn open_keys(secret_key: &[u8], eph: &DeviceBuffer, eph_pitch: u64, count: u64, keys: &mut DeviceBuffer,
                 key_pitch: u64, status: &mut DeviceBuffer, scratch: &mut DeviceBuffer, stream: Stream) -> Result<()> {
    if !pitched(eph.len(), eph_pitch, 65, count) || !pitched(keys.len(), key_pitch, 32, count) ||
        (status.len() as u64) < 4 * count || (scratch.len() as u64) < agree_scratch_len(count) {
        return Err(ChipError::InvalidArgument);
    }
    abi_agree()?;
    check(unsafe {
        ffi_agree::chipy_open_keys_dev(secret_key.as_ptr(), secret_key.len() as u64, eph.as_ptr(), eph_pitch, count,
                                       keys.as_mut_ptr(), key_pitch, status.as_mut_ptr() as *mut u32, scratch.ptr,
                                       scratch.len() as u64, stream.0)
    })
}

/// [`ecies_seal_ragged`] with the key agreement on the device: no host
/// elliptic-curve work.  `scratch` holds [`envelope_scratch_len`]`(n)` bytes.
#[allow(clippy::too_many_arguments)]
pub fn ecies_seal_ragged_dev_keys(pubkey: &[u8], input: &DeviceBuffer, in_off: &[u64], n: &[u64],
                                  out: &mut DeviceBuffer, out_off: &[u64], scratch: &mut DeviceBuffer, stream: Stream)
                                  -> Result<()> {
    let count = n.len();
    let need = envelope_scratch_len(n);
    if in_off.len() != count || out_off.len() != count || !ranges_fit(in_off, n, 0, input.len()) ||
        !ranges_fit(out_off, n, 97, out.len()) || (count > 0 && need == 0) || (scratch.len() as u64) < need {
        return Err(ChipError::InvalidArgument);
    }
    abi_agree()?;
    check(unsafe {
        ffi_agree::chipy_seal_ragged_dev(pubkey.as_ptr(), pubkey.len() as u64, ptr::null(), input.as_ptr(),
                                         in_off.as_ptr(), n.as_ptr(), count as u64, out.as_mut_ptr(), out_off.as_ptr(),
                                         scratch.ptr, stream.0)
    })
}

/// [`ecies_open_ragged`] with the key agreement on the device: no copy back
/// and no wait.  `scratch` holds [`envelope_scratch_len`] of the plaintext
/// lengths.  Returns the plaintext length per object.
#[allow(clippy::too_many_arguments)]
pub fn ecies_open_ragged_dev_keys(secret_key: &[u8], input: &DeviceBuffer, in_off: &[u64], in_len: &[u64],
                                  out: &mut DeviceBuffer, out_off: &[u64], status: &mut DeviceBuffer,
                                  scratch: &mut DeviceBuffer, stream: Stream) -> Result<Vec<u64>> {
    let count = in_len.len();
    let plain: Vec<u64> = in_len.iter().map(|&l| l.saturating_sub(97)).collect();
    let need = envelope_scratch_len(&plain);
    if in_off.len() != count || out_off.len() != count || status.len() < 4 * count ||
        !ranges_fit(in_off, in_len, 0, input.len()) || !ranges_fit(out_off, &plain, 0, out.len()) ||
        (count > 0 && need == 0) || (scratch.len() as u64) < need {
        return Err(ChipError::InvalidArgument);
    }
    abi_agree()?;
    let mut olen = vec![0u64; count];
    check(unsafe {
        ffi_agree::chipy_open_ragged_dev(secret_key.as_ptr(), secret_key.len() as u64, input.as_ptr(), in_off.as_ptr(),
                                         in_len.as_ptr(), count as u64, out.as_mut_ptr(), out_off.as_ptr(),
                                         olen.as_mut_ptr(), status.as_mut_ptr() as *mut u32, scratch.ptr, stream.0)
    })?;
    Ok(olen)
}

/// Scratch of [`encode_ragged_ecies_dev_keys`] (object lengths) / [`decode_ragged_ecies_dev_keys`] (stream lengths).
pub fn ecies_ragged_scratch_len_dev_keys(format: u8, lens: &[u64], decode: bool) -> u64 {
    unsafe {
        if decode {
            ffi_agree::chipy_decode_scratch_len(format, lens.as_ptr(), lens.len() as u64)
        } else {
            ffi_agree::chipy_encode_scratch_len(format, lens.as_ptr(), lens.len() as u64)
        }
    }
}

/// [`encode_ragged_ecies`] with the key agreement on the device.
#[allow(clippy::too_many_arguments)]
pub fn encode_ragged_ecies_dev_keys(format: u8, pubkey: &[u8], input: &DeviceBuffer, in_off: &[u64], sizes: &[u64],
                                    out: &mut DeviceBuffer, out_off: &[u64], hashes: &mut DeviceBuffer,
                                    scratch: &mut DeviceBuffer, stream: Stream)
                                    -> Result<(Vec<u64>, Vec<ChipEncodeInfo>)> {
    let count = sizes.len();
    let env: Vec<u64> = sizes.iter().map(|&n| n + 97).collect();
    let need_scratch = ecies_ragged_scratch_len_dev_keys(format, sizes, false);
    if in_off.len() != count || out_off.len() != count || hashes.len() < count * HASH_LEN || need_scratch == 0 ||
        (scratch.len() as u64) < need_scratch || !ranges_fit(in_off, sizes, 0, input.len()) {
        return Err(ChipError::InvalidArgument);
    }
    let (_, need, _) = ragged_layout(format & 12, &env, 256, 0)?;
    if !ranges_fit(out_off, &need, 0, out.len()) {
        return Err(ChipError::InvalidArgument);
    }
    abi_agree()?;
    let mut lens = vec![0u64; count];
    let mut infos = vec![ChipEncodeInfo::default(); count];
    check(unsafe {
        ffi_agree::chipy_encode_ragged_dev(format, pubkey.as_ptr(), pubkey.len() as u64, ptr::null(), input.as_ptr(),
                                           in_off.as_ptr(), sizes.as_ptr(), count as u64, out.as_mut_ptr(),
                                           out_off.as_ptr(), lens.as_mut_ptr(), hashes.as_mut_ptr(), infos.as_mut_ptr(),
                                           scratch.ptr, stream.0)
    })?;
    Ok((lens, infos))
}

/// [`decode_ragged_ecies`] with the key agreement on the device: the call no
/// longer blocks.  Returns the plaintext lengths.
#[allow(clippy::too_many_arguments)]
pub fn decode_ragged_ecies_dev_keys(format: u8, secret_key: &[u8], input: &DeviceBuffer, in_off: &[u64],
                                    in_len: &[u64], hashes: &DeviceBuffer, padding: &[u32], out: &mut DeviceBuffer,
                                    out_off: &[u64], status: &mut DeviceBuffer, scratch: &mut DeviceBuffer,
                                    stream: Stream) -> Result<Vec<u64>> {
    let count = in_len.len();
    let need_scratch = ecies_ragged_scratch_len_dev_keys(format, in_len, true);
    if in_off.len() != count || out_off.len() != count || padding.len() != count || hashes.len() < count * HASH_LEN ||
        status.len() < 4 * count || need_scratch == 0 || (scratch.len() as u64) < need_scratch ||
        !ranges_fit(in_off, in_len, 0, input.len()) || !ranges_fit(out_off, in_len, 0, out.len()) {
        return Err(ChipError::InvalidArgument);
    }
    abi_agree()?;
    let mut olen = vec![0u64; count];
    check(unsafe {
        ffi_agree::chipy_decode_ragged_dev(format, secret_key.as_ptr(), secret_key.len() as u64, input.as_ptr(),
                                           in_off.as_ptr(), in_len.as_ptr(), count as u64, hashes.as_ptr(),
                                           padding.as_ptr(), out.as_mut_ptr(), out_off.as_ptr(), olen.as_mut_ptr(),
                                           status.as_mut_ptr() as *mut u32, scratch.ptr, stream.0)
    })?;
    Ok(olen)
}

/// Scratch of [`key_table_from_streams`] over the table `info` describes; 0 where the call would refuse it.
pub fn key_table_from_streams_scratch_len(info: &TableInfo) -> u64 {
    unsafe { ffi_agree::chipy_key_table_scratch_len(info) }
}

/// The key table of the resident level-13 streams a stream table describes,
/// made without the host seeing a header or a key: what [`stream_keys`]
/// followed by [`key_table`] produce, byte for byte, from a strict vouched
/// planned read of every envelope's first 81 bytes and the key agreement
/// kernels.  No copy back, no wait; the only upload is the secret.  Enqueued on
/// `stream`.
pub fn key_table_from_streams(stream_table: &DeviceBuffer, info: &TableInfo, secret_key: &[u8],
                              table: &mut DeviceBuffer, scratch: &mut DeviceBuffer, stream: Stream) -> Result<()> {
    let need = key_table_from_streams_scratch_len(info);
    if (table.len() as u64) < key_table_len(info.nstreams) || (info.nstreams > 0 && need == 0) ||
        (scratch.len() as u64) < need {
        return Err(ChipError::InvalidArgument);
    }
    abi_agree()?;
    check(unsafe {
        ffi_agree::chipy_key_table_dev(stream_table.ptr, info, secret_key.as_ptr(), secret_key.len() as u64, table.ptr,
                                       table.len() as u64, scratch.ptr, scratch.len() as u64, stream.0)
    })
}

#[cfg(test)]
mod tests {
    use super::*;

    #[test]
    fn status_round_trip() {
        for s in [1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16, 17, 18, 19, 20, 100, 101] {
            assert_eq!(ChipError::from_status(s, 31, 7).status(), s);
        }
    }

    #[test]
    fn size_helpers() {
        assert_eq!(calc_padding_len(16 << 20, 4).unwrap(), (0, 4 << 20));
        assert_eq!(bao_encoded_len(16 << 20), 35_651_528);
        assert_eq!(zfec_encoded_len(1243, 4, 8), 8192);
    }

    #[test]
    fn layouts_match_the_header() {
        assert_eq!(std::mem::size_of::<ChipEncodeInfo>(), 44);
        assert_eq!(std::mem::size_of::<ffi::chip_ecies_inject>(), 16);
        assert_eq!(std::mem::size_of::<ChipHeader>(), 152);
    }
}
