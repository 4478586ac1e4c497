// picotls_amd/csrc/aesgcm_engine.hip -- MI355X (gfx950 / CDNA4) AES-GCM record engine: HIP kernels + the C ABI
// declared in include/picotls/mi355x.h.
//
// What it replaces: picotls' fusion AES-GCM engine (lib/fusion.c:401-845 seal/open, :847-929 AES core and key
// schedule, :114-321 + :934-1011 GHASH and H-power tables), re-designed for a GPU: one launch seals or opens a
// whole batch of independent records.
//
// Design (DESIGN.md has the numbers):
//   * one persistent 1024-thread workgroup per CU; G = 8 lanes of a wavefront work on one record, so a wave holds 8
//     records and lane j of a record handles GHASH stream positions j, j+G, j+2G, ... (the stream is
//     [zero padding | AAD blocks | ciphertext blocks | length block], front-padded to a multiple of G, which leaves
//     GHASH unchanged). A record's ciphertext block b sits at one stream position, so the lane that runs AES-CTR
//     on counter 2+b is the lane that folds that block into its GHASH accumulator: no data exchange.
//   * AES: T-table rounds from LDS. Te0 and Te2 (= rotl16 Te0) are replicated into all 32 banks
//     (entry n at n*256 + bank*4, Te2 at +128): lane l always reads bank l%32, so every ds_read_b32 is
//     conflict-free; Te1/Te3 are one v_alignbit away. The byte -> LDS address step is a single v_perm_b32.
//   * GHASH: 4-bit-window tables in LDS. For each H power one table = 32 windows x 16 entries x 16 B (8 KiB);
//     the 16 entries of a window fill exactly one 256-byte LDS bank row, so a ds_read_b128 of 16 lanes never
//     conflicts (equal entries broadcast). A product X*H^k is the XOR of 32 table entries; the reduction is baked
//     into the tables. Horner with stride H^G on every step except the last, where lane j multiplies by H^(G-j)
//     instead; an XOR over the G lanes then gives GHASH. Tables for H^1..H^G (64 KiB) are built on chip from the
//     keyset's H powers at kernel start.
//   * Data path: 16-byte unaligned-capable global loads/stores (unaligned access mode is on for gfx950), G lanes
//     of a record touch G*16 contiguous bytes per step. Partial first/last blocks use byte accesses so nothing
//     outside [in_off, in_off+len) / [out_off, out_off+len+16) is touched.
//
// All word-level state is kept in "LE column" form: a 16-byte block is 4 little-endian u32 words, word c = bytes
// 4c..4c+3 = AES state column c. GHASH elements use the same byte order (byte 0 holds x^0..x^7, MSB first).

#include <hip/hip_runtime.h>
#include <algorithm>
#include <atomic>
#include <chrono>
#include <functional>
#include <mutex>
#include <new>
#include <type_traits>
#include <utility>
#include <vector>
#include <stdlib.h>
#include <stdint.h>
#include <string.h>
#include <stdio.h>
#include <sched.h>

#include "picotls/mi355x.h"
#include "picotls/mi355x_debug.h"
#include "picotls/mi355x_quic.h"

// Device code, in dependency order (one translation unit: the kernels are templates instantiated by the host side)
#include "engine/common.h"
#include "engine/keyset_setup.h"
#include "engine/lds_tables.h"
#include "engine/aes_tt.h"
#include "engine/ghash.h"
#include "engine/record.h"
#include "engine/segment.h"
#include "engine/gcm_kernels.h"
#include "quic/header.h"  // (suite-neutral: the ChaCha20 kernels below use it too)
#include "engine/aux_kernels.h"
#include "engine/lane_kernels.h"
#include "engine/span_kernels.h"

// ------------------------------------------------------------------------------------------------ host side
// (host/runtime.h: what both AEAD families share; host/aesgcm.h: the AES-GCM keyset, launches and C ABI)
#include "host/runtime.h"
#include "host/aesgcm.h"

// ------------------------------------------------------------------------------------------------ ChaCha20-Poly1305
// The second AEAD family (include/picotls/mi355x_chacha20.h), in this translation unit so that its host side shares
// host/runtime.h. Nothing above depends on it.
#include "picotls/mi355x_chacha20.h"
#include "chacha/chacha20.h"
#include "chacha/poly1305.h"
#include "chacha/kernels.h"
#include "chacha/host.h"
