"""EVP AES-256-GCM (16-byte IV, no AAD) through ctypes on the libcrypto the
library already links, and GCM's J0 on Python integers: the reference of the
GPU tests of the AES-GCM kernels, which shares nothing with the bitsliced AES
and the table-free GHASH under test."""
import ctypes
import ctypes.util

_C = ctypes.CDLL(ctypes.util.find_library("crypto") or "libcrypto.so.3")
_C.EVP_CIPHER_CTX_new.restype = ctypes.c_void_p
_C.EVP_aes_256_gcm.restype = ctypes.c_void_p
_C.EVP_aes_256_ecb.restype = ctypes.c_void_p
_GCM_SET_IVLEN, _GCM_GET_TAG = 0x9, 0x10


def evp_seal(key: bytes, iv: bytes, pt: bytes):
    """(ciphertext, tag) of EVP AES-256-GCM with a 16-byte IV and no AAD."""
    ctx = ctypes.c_void_p(_C.EVP_CIPHER_CTX_new())
    out = ctypes.create_string_buffer(len(pt) + 16)
    n, tag = ctypes.c_int(0), ctypes.create_string_buffer(16)
    try:
        assert _C.EVP_EncryptInit_ex(ctx, ctypes.c_void_p(_C.EVP_aes_256_gcm()), None, None, None) == 1
        assert _C.EVP_CIPHER_CTX_ctrl(ctx, _GCM_SET_IVLEN, 16, None) == 1
        assert _C.EVP_EncryptInit_ex(ctx, None, None, key, iv) == 1
        total = 0
        if pt:
            assert _C.EVP_EncryptUpdate(ctx, out, ctypes.byref(n), pt, len(pt)) == 1
            total = n.value
        fin = ctypes.create_string_buffer(16)
        assert _C.EVP_EncryptFinal_ex(ctx, fin, ctypes.byref(n)) == 1 and n.value == 0
        assert _C.EVP_CIPHER_CTX_ctrl(ctx, _GCM_GET_TAG, 16, tag) == 1
    finally:
        _C.EVP_CIPHER_CTX_free(ctx)
    assert total == len(pt)
    return out.raw[:total], tag.raw


def evp_ecb(key: bytes, block: bytes) -> bytes:
    ctx = ctypes.c_void_p(_C.EVP_CIPHER_CTX_new())
    out, n = ctypes.create_string_buffer(32), ctypes.c_int(0)
    try:
        assert _C.EVP_EncryptInit_ex(ctx, ctypes.c_void_p(_C.EVP_aes_256_ecb()), None, key, None) == 1
        _C.EVP_CIPHER_CTX_set_padding(ctx, 0)
        assert _C.EVP_EncryptUpdate(ctx, out, ctypes.byref(n), block, 16) == 1
    finally:
        _C.EVP_CIPHER_CTX_free(ctx)
    return out.raw[:16]


def gf128_mul(x: int, y: int) -> int:
    """SP 800-38D algorithm 1 on Python integers (bit 127 = the block's first bit)."""
    z, v = 0, y
    for i in range(128):
        if (x >> (127 - i)) & 1:
            z ^= v
        v = (v >> 1) ^ (0xE1 << 120) if v & 1 else v >> 1
    return z


def j0_of(key: bytes, iv: bytes) -> int:
    h = int.from_bytes(evp_ecb(key, bytes(16)), "big")
    return gf128_mul(gf128_mul(int.from_bytes(iv, "big"), h) ^ 128, h)
