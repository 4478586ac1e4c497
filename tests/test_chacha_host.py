"""CPU-side checks of the ChaCha20-Poly1305 engine: the three references agree, and the boundary of
include/picotls/mi355x_chacha20.h is what the package and the shared objects say it is. No device calls."""
import os
import re
import subprocess

import numpy as np
import pytest

import chacha_ref as R
import picotls_amd as pa

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def declared(header: str) -> set:
    text = open(os.path.join(ROOT, "include", "picotls", header)).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return set(re.findall(r"\b(ptls_mi355x_\w+)\s*\(", text))


def exported(so: str) -> set:
    out = subprocess.run(["nm", "-D", "--defined-only", so], capture_output=True, text=True, check=True).stdout
    return {line.split()[-1] for line in out.splitlines() if line.strip()}


def test_rfc_aead_vectors_on_both_references():
    for v in R.load_kat()["aead"]:
        key, nonce, aad, pt = (bytes.fromhex(v[k]) for k in ("key", "nonce", "aad", "plaintext"))
        sealed = bytes.fromhex(v["ciphertext"] + v["tag"])
        assert R.ossl_seal(key, nonce, pt, aad) == sealed, v["name"]
        assert R.py_seal(key, nonce, pt, aad) == sealed, v["name"]
        assert R.ossl_open(key, nonce, sealed, aad) == pt
        assert R.py_open(key, nonce, sealed, aad) == pt
        bad = bytes([sealed[0] ^ 0xff]) + sealed[1:]
        assert R.ossl_open(key, nonce, bad, aad) is None and R.py_open(key, nonce, bad, aad) is None


def test_rfc_poly1305_vectors_on_the_python_reference():
    vs = R.load_kat()["poly1305"]
    assert len(vs) == 12
    for v in vs:
        assert R.py_poly1305(bytes.fromhex(v["r"] + v["s"]), bytes.fromhex(v["msg"])) == bytes.fromhex(v["tag"]), v


def test_openssl_and_python_agree_on_every_length():
    rng = np.random.default_rng(8439)
    key, iv = rng.bytes(32), rng.bytes(12)
    for i, n in enumerate(list(range(300)) + [1200, 4096, 16384, 16385]):
        pt, aad = rng.bytes(n), rng.bytes(i % 41)
        nonce = R.nonce_for(iv, int(rng.integers(0, 2**62)))
        a = R.ossl_seal(key, nonce, pt, aad)
        if n < 300 or n == 1200:  # (the bigint restatement takes ~10 ms per KiB)
            assert R.py_seal(key, nonce, pt, aad) == a, n
        assert R.ossl_open(key, nonce, a, aad) == pt, n


def test_openssl_chacha20_is_counter_then_nonce():
    rng = np.random.default_rng(20)
    key, iv16 = rng.bytes(32), rng.bytes(16)
    block = R.py_chacha20_block(key, int.from_bytes(iv16[:4], "little"), iv16[4:])
    assert R.ossl_chacha20(key, iv16, bytes(16)) == block[:16]


def test_nonce_is_static_iv_xor_big_endian_seq():
    assert R.nonce_for(bytes(range(12)), 0x0102030405060708) == bytes([0, 1, 2, 3, 4 ^ 1, 5 ^ 2, 6 ^ 3, 7 ^ 4, 8 ^ 5, 9 ^ 6, 10 ^ 7, 11 ^ 8])


def test_chacha_header_is_the_python_boundary():
    decl = declared("mi355x_chacha20.h")
    assert decl == set(pa.CHACHA_ABI_FUNCTIONS)
    assert len(pa.CHACHA_ABI_FUNCTIONS) == len(set(pa.CHACHA_ABI_FUNCTIONS))
    assert not decl & set(pa.ABI_FUNCTIONS)
    assert not decl & set(pa.DEBUG_FUNCTIONS)
    missing = decl - exported(pa.LIB_PATH)
    assert not missing, missing
    lib = pa.load_library()
    for name in pa.CHACHA_ABI_FUNCTIONS:
        assert getattr(lib, name) is not None


def test_picotls_backend_exports_chacha_objects():
    if not os.path.exists(pa.PICOTLS_LIB_PATH):
        pytest.skip("picotls headers were not available at build time")
    syms = exported(pa.PICOTLS_LIB_PATH)
    assert {"ptls_mi355x_chacha20", "ptls_mi355x_chacha20poly1305"} <= syms
    assert declared("mi355x_chacha20_picotls.h") <= syms
    text = open(os.path.join(ROOT, "include", "picotls", "mi355x_chacha20_picotls.h")).read()
    assert re.search(r"extern\s+ptls_cipher_algorithm_t\s+ptls_mi355x_chacha20;", text)
    assert re.search(r"extern\s+ptls_aead_algorithm_t\s+ptls_mi355x_chacha20poly1305;", text)


def test_algorithm_descriptor_matches_picotls():
    a = pa.chacha20poly1305
    assert (a.name, a.key_size, a.iv_size, a.tag_size) == ("CHACHA20-POLY1305", 32, 12, 16)
    assert a.confidentiality_limit == 2**64 - 1 and a.integrity_limit == 2**36
    assert (a.tls12_fixed_iv_size, a.tls12_record_iv_size) == (12, 0)
    assert pa.CHACHA_GROUP_WIDTHS == (4, 16)


@pytest.mark.parametrize("keys, ivs", [(b"", b""), (bytes(31), bytes(12)), (bytes(33), bytes(12)), (bytes(32), bytes(11)),
                                       (bytes(64), bytes(12)), (bytes(32), bytes(24)), (bytes(16), bytes(12))])
def test_keyset_rejects_bad_sizes_before_any_device_call(keys, ivs):
    with pytest.raises(ValueError):
        pa.ChaChaKeyset(keys, ivs)


def test_contexts_reject_bad_sizes_before_any_device_call():
    with pytest.raises(ValueError):
        pa.AeadContext(pa.chacha20poly1305, True, bytes(16), bytes(12))
    with pytest.raises(ValueError):
        pa.AeadContext(pa.chacha20poly1305, True, bytes(32), bytes(8))
    with pytest.raises(ValueError):
        pa.ChaChaCipher(bytes(16))
    with pytest.raises(ValueError):
        pa.chacha_debug_poly1305(bytes(31), b"")


def test_new_sources_enter_the_engine_digest():
    from picotls_amd import build as b

    csrc = os.path.join(b.PKG, "csrc")
    on_disk = {os.path.join(d, f) for d, _, files in os.walk(csrc) for f in files if f.endswith(".h")}
    assert {os.path.join(csrc, "chacha", "host.h"), os.path.join(csrc, "host", "runtime.h"),
            os.path.join(csrc, "engine", "common.h")} <= on_disk
    assert on_disk <= set(b.ENGINE_PARTS)  # every header below csrc/, whatever its directory
    assert os.path.join(ROOT, "include", "picotls", "mi355x_chacha20.h") in b.HEADERS
    # every quoted #include of the translation unit resolves to a file the digest covers
    covered = {os.path.realpath(p) for p in b.ENGINE_SRCS + b.ENGINE_PARTS + b.HEADERS}
    for src in b.ENGINE_SRCS + b.ENGINE_PARTS:
        for inc in re.findall(r'^\s*#\s*include\s+"([^"]+)"', open(src).read(), flags=re.M):
            found = [p for p in (os.path.join(os.path.dirname(src), inc), os.path.join(csrc, inc), os.path.join(ROOT, "include", inc))
                     if os.path.exists(p)]
            assert found, f"{src} includes {inc}, which is not in the tree"
            assert os.path.realpath(found[0]) in covered, f"{src} includes {inc}, which the engine digest does not cover"
