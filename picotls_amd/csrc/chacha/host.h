// picotls_amd/csrc/chacha/host.h -- host side of the ChaCha20-Poly1305 engine: the C ABI of
// include/picotls/mi355x_chacha20.h. Part of the single translation unit picotls_amd/csrc/aesgcm_engine.hip, included
// last: built on host/runtime.h (per-device state, streams, event pool, StreamUses, Scratch, StreamSlots, StageCall, error reporting).
#ifndef PTLS_MI355X_CHACHA_HOST_H
#define PTLS_MI355X_CHACHA_HOST_H

#define CHACHA_WG_PER_CU 4    // launch grid: this many 256-thread workgroups per CU at most (what ~120 VGPRs a lane keep resident)
#define CHACHA_CLAIM_SLOTS 8  // claim counters per keyset: one per stream in use, shared in stream order beyond that
#define CHACHA_SPREAD_WG_PER_CU 2  // grid of a spread launch of a batch (the host cannot count its pieces)

// A keyset is the entry array and, behind it, its claim counters (a pair of u64 per slot, zero between launches).
// Launches on one stream run in order and share a slot; a stream without one takes a free slot, or takes the least
// recently used one over after waiting for the last launch of the stream that held it (StreamSlots).
struct st_ptls_mi355x_chacha_keyset_t {
    DeviceState *ds = nullptr;
    int device = 0;
    size_t nkeys = 0;
    ChaChaKey *d_keys = nullptr;
    unsigned long long *d_claim = nullptr;
    // spread launches: per claim slot the records' accumulators (CHACHA_SPREAD_SCRATCH_BYTES, zero between launches),
    // allocated in the order of the slot's stream on first use (Scratch); a stream that takes a slot over waits as for
    // the claim
    Scratch spread[CHACHA_CLAIM_SLOTS];
    std::vector<uint8_t> ivs;  // the static IVs (get_iv reads these; the device copy is what seals use)
    std::mutex mu;             // launches from several threads: the two below, held from taking a slot through the
                               // launch and the use event after it
    StreamUses uses;           // per stream: after this keyset's last launch on it (teardown and rekey wait for these)
    StreamSlots<unsigned, CHACHA_CLAIM_SLOTS> slots;  // per stream: the index of its claim slot
};

static std::atomic<u32> g_chacha_force_g{0}, g_chacha_force_wgs{0};
static std::atomic<u32> g_chacha_spread_piece{0}, g_chacha_spread_min{0}, g_chacha_spread_force{0};  // debug_spread

// `launch()` on `s` and the keyset's use after it (ks->mu held); a launch error is reported through `fmt`. A launch that
// reads a second keyset too (QUIC packets: `hp_ks`, its mutex held as well) is a use of both.
template <typename Launch>
static int chacha_launch_noted(ptls_mi355x_chacha_keyset_t *ks, hipStream_t s, const char *fmt, Launch launch,
                               ptls_mi355x_chacha_keyset_t *hp_ks = nullptr)
{
    return launch_and_note_both(ks, hp_ks != nullptr ? hp_ks : ks, s, [&] {
        LAUNCH_CLEAR();
        launch();
        const hipError_t e = hipGetLastError();
        return e == hipSuccess ? 0 : fail(fmt, hipGetErrorString(e));
    });
}

static std::vector<ChaChaKey> chacha_entries(const void *keys, const void *ivs, size_t n)  // (the caller clears them)
{
    std::vector<ChaChaKey> host(n);
    for (size_t i = 0; i < n; ++i) {
        memset(&host[i], 0, sizeof(ChaChaKey));
        memcpy(host[i].key, (const uint8_t *)keys + i * 32, 32);
        memcpy(host[i].iv, (const uint8_t *)ivs + i * 12, 12);
    }
    return host;
}

static unsigned chacha_grid(const DeviceState *ds, size_t nrecs)
{
    u64 grid = (nrecs + CHACHA_WG / CHACHA_G_WIDE - 1) / (CHACHA_WG / CHACHA_G_WIDE);
    grid = min(grid, (u64)ds->ncu * CHACHA_WG_PER_CU);
    const u32 cap = g_chacha_force_wgs.load(std::memory_order_relaxed);
    if (cap != 0)
        grid = min(grid, (u64)cap);
    return (unsigned)grid;
}

static void chacha_launch_kernel(bool open, int frame, unsigned grid, hipStream_t s, const ChaChaArgs &a)
{
    const auto go = [&](auto FRAME) {
        with_bool(open, [&](auto OPEN) { chacha_batch_kernel<OPEN, FRAME><<<grid, CHACHA_WG, 0, s>>>(a); });
    };
    if (frame == 2)  // QUIC packets
        go(std::integral_constant<int, 2>{});
    else
        with_either<0, 1>(frame, go);
}

// the accumulators of claim slot `slot` for a spread launch on `s` (ks->mu held), all zero when allocated; nullptr on
// failure, which fails the call
static unsigned long long *chacha_spread_scratch(ptls_mi355x_chacha_keyset_t *ks, unsigned slot, hipStream_t s)
{
    return (unsigned long long *)ks->spread[slot].take(ks->ds, ks->uses, s, CHACHA_SPREAD_SCRATCH_BYTES, CHACHA_SPREAD_SCRATCH_BYTES);
}

// whether a launch may be a spread one: a forced group width keeps it on chacha_batch_kernel unless debug_spread forces
static bool chacha_spread_allowed(u32 force_g) { return force_g == 0 || g_chacha_spread_force.load(std::memory_order_relaxed) != 0; }

static u32 chacha_spread_base_piece(void)
{
    const u32 p = g_chacha_spread_piece.load(std::memory_order_relaxed);
    return p != 0 ? p : CHACHA_SPREAD_PIECE;
}

static u32 chacha_spread_min_len(u32 compiled)
{
    const u32 m = g_chacha_spread_min.load(std::memory_order_relaxed);
    return m != 0 ? m : compiled;
}

// the grid of a spread launch: the workgroups its pieces need where the host knows them (`want`, a lone record), at
// most CHACHA_SPREAD_WG_PER_CU a CU
static unsigned chacha_spread_grid(const DeviceState *ds, size_t want)
{
    size_t grid = std::min<size_t>(want, (size_t)ds->ncu * CHACHA_SPREAD_WG_PER_CU);
    const u32 cap = g_chacha_force_wgs.load(std::memory_order_relaxed);
    if (cap != 0)
        grid = std::min<size_t>(grid, cap);
    return (unsigned)std::max<size_t>(grid, 1);
}

static void chacha_launch_spread(bool open, unsigned grid, hipStream_t s, const ChaChaSpreadArgs &sa)
{
    with_bool(open, [&](auto OPEN) { chacha_spread_kernel<OPEN><<<grid, CHACHA_WG, 0, s>>>(sa); });
}

static int chacha_launch_batch(ptls_mi355x_chacha_keyset_t *ks, bool open, int frame, const ptls_mi355x_record_t *recs, size_t nrecs,
                               const void *in, const void *aad, void *out, uint8_t *ok, void *stream)
{
    if (ks == NULL || (nrecs != 0 && (recs == NULL || in == NULL || out == NULL || (open && ok == NULL))))
        return fail("%s", "chacha batch: invalid arguments");
    if (nrecs == 0)
        return 0;
    DeviceScope scope(ks->device);
    hipStream_t s = (hipStream_t)stream;
    std::lock_guard<std::mutex> lk(ks->mu);
    const unsigned *slot = ks->slots.get(s, ks->uses, [&](unsigned &i) { return i = (unsigned)ks->slots.v.size(), true; });
    if (slot == nullptr)
        return -1;
    ChaChaArgs a = {};
    a.keys = ks->d_keys, a.nkeys = (u32)ks->nkeys, a.force_g = g_chacha_force_g.load(std::memory_order_relaxed);
    a.recs = recs, a.nrecs = nrecs, a.in = (const uint8_t *)in, a.aad = (const uint8_t *)aad, a.out = (uint8_t *)out, a.ok = ok;
    // a small unframed batch: its long records spread over the device (chacha_spread_kernel)
    if (frame == 0 && nrecs <= CHACHA_SPREAD_MAX_RECS && chacha_spread_allowed(a.force_g)) {
        ChaChaSpreadArgs sa = {};
        sa.a = a, sa.piece = chacha_spread_base_piece(), sa.min_len = chacha_spread_min_len(CHACHA_SPREAD_MIN_BATCH);
        if ((sa.acc = chacha_spread_scratch(ks, *slot, s)) == nullptr)
            return -1;
        const unsigned sgrid = chacha_spread_grid(ks->ds, SIZE_MAX);  // (the host cannot count the batch's pieces)
        return chacha_launch_noted(ks, s, "chacha spread launch: %s", [&] { chacha_launch_spread(open, sgrid, s, sa); });
    }
    a.claim = ks->d_claim + 2 * *slot;
    const unsigned grid = chacha_grid(ks->ds, nrecs);
    return chacha_launch_noted(ks, s, "chacha batch launch: %s", [&] { chacha_launch_kernel(open, frame, grid, s, a); });
}

// QUIC packets: one launch (seal), or the header pre-pass and the batch behind it on the same stream (open). The launch
// reads both keysets: PairLock and launch_and_note_both (host/runtime.h).
static int chacha_launch_quic(ptls_mi355x_chacha_keyset_t *ks, ptls_mi355x_chacha_keyset_t *hp_ks, bool open,
                              const ptls_mi355x_record_t *recs, size_t nrecs, const void *in, void *out, uint8_t *ok,
                              ptls_mi355x_quic_result_t *results, void *stream)
{
    if (check_quic_args("chacha quic packets", ks, hp_ks, open, recs, nrecs, in, out, ok, results) != 0)
        return -1;
    if (nrecs == 0)
        return 0;
    DeviceScope scope(ks->device);
    hipStream_t s = (hipStream_t)stream;
    PairLock<ptls_mi355x_chacha_keyset_t> locks(ks, hp_ks);
    const unsigned *slot = ks->slots.get(s, ks->uses, [&](unsigned &i) { return i = (unsigned)ks->slots.v.size(), true; });
    if (slot == nullptr)
        return -1;
    ChaChaArgs a = {};
    a.keys = ks->d_keys, a.nkeys = (u32)ks->nkeys, a.force_g = g_chacha_force_g.load(std::memory_order_relaxed);
    a.recs = recs, a.nrecs = nrecs, a.in = (const uint8_t *)in, a.out = (uint8_t *)out, a.ok = ok;
    a.claim = ks->d_claim + 2 * *slot;
    a.hp_keys = hp_ks->d_keys, a.hp_nkeys = (u32)hp_ks->nkeys, a.results = results;
    const unsigned grid = chacha_grid(ks->ds, nrecs);
    return chacha_launch_noted(ks, s, "chacha quic packets launch: %s", [&] {
        if (open)
            chacha_quic_unmask_kernel<<<aux_grid(nrecs, ks->ds->ncu), 256, 0, s>>>(a.hp_keys, a.hp_nkeys, a.nkeys, recs, nrecs, a.in, results);
        chacha_launch_kernel(open, 2, grid, s, a);
    }, hp_ks);
}

extern "C" {

ptls_mi355x_chacha_keyset_t *ptls_mi355x_chacha_keyset_new(const void *keys, const void *ivs, size_t nkeys)
{
    if (keys == NULL || ivs == NULL || nkeys == 0 || nkeys > (1u << 30)) {
        fail("%s", "ptls_mi355x_chacha_keyset_new: invalid arguments");
        return NULL;
    }
    DeviceState *ds = current_device_state();
    if (ds == nullptr)
        return NULL;
    ptls_mi355x_chacha_keyset_t *ks = new (std::nothrow) st_ptls_mi355x_chacha_keyset_t();
    if (ks == nullptr) {
        fail("%s", "out of memory");
        return NULL;
    }
    ks->ds = ds, ks->device = ds->device, ks->nkeys = nkeys;
    ks->ivs.assign((const uint8_t *)ivs, (const uint8_t *)ivs + nkeys * 12);
    std::vector<ChaChaKey> host = chacha_entries(keys, ivs, nkeys);
    free_after_maint(ds, nullptr);  // (entries of freed keysets whose clearing has run go back to the pool)
    // entries and counters in stream-ordered memory on the setup stream; the call waits for that stream only
    const size_t kbytes = nkeys * sizeof(ChaChaKey), cbytes = CHACHA_CLAIM_SLOTS * 2 * sizeof(unsigned long long);
    const bool ok = hipMallocAsync((void **)&ks->d_keys, kbytes + cbytes, ds->setup) == hipSuccess &&
                    hipMemcpyAsync(ks->d_keys, host.data(), kbytes, hipMemcpyHostToDevice, ds->setup) == hipSuccess &&
                    hipMemsetAsync((uint8_t *)ks->d_keys + kbytes, 0, cbytes, ds->setup) == hipSuccess &&
                    hipStreamSynchronize(ds->setup) == hipSuccess;
    clear_memory(host.data(), kbytes);
    if (!ok) {
        (void)hipGetLastError();
        if (ks->d_keys != nullptr)
            (void)hipFreeAsync(ks->d_keys, ds->setup);
        clear_memory(ks->ivs.data(), ks->ivs.size());
        delete ks;
        fail("%s", "ptls_mi355x_chacha_keyset_new: device setup failed");
        return NULL;
    }
    ks->d_claim = (unsigned long long *)((uint8_t *)ks->d_keys + kbytes);
    return ks;
}

void ptls_mi355x_chacha_keyset_free(ptls_mi355x_chacha_keyset_t *ks)
{
    if (ks == NULL)
        return;
    DeviceScope scope(ks->device);
    DeviceState *ds = ks->ds;
    // the key material is cleared after the keyset's last launch, on the maintenance stream; where that order cannot be
    // set up on the device the host waits for the launches instead, and failing that too the entries are left as they are
    if (std::lock_guard<std::mutex> lk(ks->mu); ks->uses.order_after_all(ds->maint) == 0 || ks->uses.drain()) {
        (void)hipMemsetAsync(ks->d_keys, 0, ks->nkeys * sizeof(ChaChaKey), ds->maint);
        free_after_maint(ds, ks->d_keys);
        for (Scratch &acc : ks->spread)
            acc.release(ds, true);
    }
    ks->uses.release(ds);
    clear_memory(ks->ivs.data(), ks->ivs.size());
    delete ks;
}

size_t ptls_mi355x_chacha_keyset_size(const ptls_mi355x_chacha_keyset_t *ks) { return ks->nkeys; }
int ptls_mi355x_chacha_keyset_device(const ptls_mi355x_chacha_keyset_t *ks) { return ks->device; }

int ptls_mi355x_chacha_keyset_update(ptls_mi355x_chacha_keyset_t *ks, const uint32_t *key_idx, const void *keys, const void *ivs,
                                     size_t n)
{
    if (ks == NULL || (n != 0 && (key_idx == NULL || keys == NULL || ivs == NULL)))
        return fail("%s", "chacha keyset_update: invalid arguments");
    if (check_update_indices("chacha keyset_update", key_idx, n, ks->nkeys) != 0)
        return -1;
    if (n == 0)
        return 0;
    DeviceScope scope(ks->device);
    DeviceState *ds = ks->ds;
    std::vector<ChaChaKey> host = chacha_entries(keys, ivs, n);
    // on the maintenance stream, after every launch already made with the old entries; the call returns once the
    // scatter has run, so launches made after it see the new ones
    if (std::lock_guard<std::mutex> lk(ks->mu); ks->uses.order_after_all(ds->maint) != 0)
        return -1;
    uint8_t *d = NULL;
    const size_t kb = n * sizeof(ChaChaKey), sb = n * 4;
    HIP_TRY(hipMallocAsync((void **)&d, kb + sb, ds->maint));
    int ret = -1;
    if (hipMemcpyAsync(d, host.data(), kb, hipMemcpyHostToDevice, ds->maint) == hipSuccess &&
        hipMemcpyAsync(d + kb, key_idx, sb, hipMemcpyHostToDevice, ds->maint) == hipSuccess) {
        LAUNCH_CLEAR();
        chacha_keys_scatter_kernel<<<(unsigned)((n + 255) / 256), 256, 0, ds->maint>>>((const ChaChaKey *)d, (const u32 *)(d + kb),
                                                                                      ks->d_keys, (u32)n);
        if (hipGetLastError() == hipSuccess)
            ret = 0;
    }
    (void)hipMemsetAsync(d, 0, kb, ds->maint);
    (void)hipFreeAsync(d, ds->maint);
    if (hipStreamSynchronize(ds->maint) != hipSuccess)
        ret = -1;
    clear_memory(host.data(), kb);
    if (ret != 0)
        return fail("%s", "chacha keyset_update: device update failed");
    for (size_t i = 0; i < n; ++i)
        memcpy(ks->ivs.data() + (size_t)key_idx[i] * 12, (const uint8_t *)ivs + i * 12, 12);
    return 0;
}

int ptls_mi355x_chacha_keyset_get_iv(ptls_mi355x_chacha_keyset_t *ks, size_t key_idx, void *iv)
{
    if (ks == NULL || key_idx >= ks->nkeys || iv == NULL)
        return fail("%s", "chacha get_iv: bad key index");
    memcpy(iv, ks->ivs.data() + key_idx * 12, 12);
    return 0;
}

int ptls_mi355x_chacha_keyset_set_iv(ptls_mi355x_chacha_keyset_t *ks, size_t key_idx, const void *iv)
{
    if (ks == NULL || key_idx >= ks->nkeys || iv == NULL)
        return fail("%s", "chacha set_iv: bad key index");
    DeviceScope scope(ks->device);
    if (std::lock_guard<std::mutex> lk(ks->mu); ks->uses.order_after_all(ks->ds->maint) != 0)
        return -1;
    HIP_TRY(hipMemcpyAsync(ks->d_keys[key_idx].iv, iv, 12, hipMemcpyHostToDevice, ks->ds->maint));
    HIP_TRY(hipStreamSynchronize(ks->ds->maint));
    memcpy(ks->ivs.data() + key_idx * 12, iv, 12);
    return 0;
}

int ptls_mi355x_chacha_seal_batch(ptls_mi355x_chacha_keyset_t *ks, const ptls_mi355x_record_t *recs, size_t nrecs, const void *in,
                                  const void *aad, void *out, void *stream)
{
    return chacha_launch_batch(ks, false, 0, recs, nrecs, in, aad, out, NULL, stream);
}

int ptls_mi355x_chacha_open_batch(ptls_mi355x_chacha_keyset_t *ks, const ptls_mi355x_record_t *recs, size_t nrecs, const void *in,
                                  const void *aad, void *out, uint8_t *ok, void *stream)
{
    return chacha_launch_batch(ks, true, 0, recs, nrecs, in, aad, out, ok, stream);
}

int ptls_mi355x_chacha_seal_tls_records(ptls_mi355x_chacha_keyset_t *ks, const ptls_mi355x_record_t *recs, size_t nrecs,
                                        const void *in, void *out, void *stream)
{
    return chacha_launch_batch(ks, false, 1, recs, nrecs, in, NULL, out, NULL, stream);
}

int ptls_mi355x_chacha_open_tls_records(ptls_mi355x_chacha_keyset_t *ks, const ptls_mi355x_record_t *recs, size_t nrecs,
                                        const void *in, void *out, uint8_t *ok, ptls_mi355x_tls_result_t *results, void *stream)
{
    if (chacha_launch_batch(ks, true, 1, recs, nrecs, in, NULL, out, ok, stream) != 0)
        return -1;
    if (nrecs == 0)
        return 0;
    DeviceScope scope(ks->device);
    LAUNCH_CLEAR();
    // header check and padding strip: the same pass as after an AES-GCM open
    tls_unpad_kernel<<<aux_grid(nrecs, ks->ds->ncu), 256, 0, (hipStream_t)stream>>>(recs, nrecs, (const uint8_t *)in,
                                                                                     (const uint8_t *)out, ok, results);
    HIP_TRY(hipGetLastError());
    return 0;
}

int ptls_mi355x_chacha_seal_quic_packets(ptls_mi355x_chacha_keyset_t *ks, ptls_mi355x_chacha_keyset_t *hp_ks,
                                         const ptls_mi355x_record_t *recs, size_t nrecs, const void *in, void *out, void *stream)
{
    return chacha_launch_quic(ks, hp_ks, false, recs, nrecs, in, out, NULL, NULL, stream);
}

int ptls_mi355x_chacha_open_quic_packets(ptls_mi355x_chacha_keyset_t *ks, ptls_mi355x_chacha_keyset_t *hp_ks,
                                         const ptls_mi355x_record_t *recs, size_t nrecs, const void *in, void *out, uint8_t *ok,
                                         ptls_mi355x_quic_result_t *results, void *stream)
{
    return chacha_launch_quic(ks, hp_ks, true, recs, nrecs, in, out, ok, results, stream);
}

int ptls_mi355x_chacha_hp_mask_batch(ptls_mi355x_chacha_keyset_t *hp_ks, const ptls_mi355x_hp_t *hp, size_t n, const void *base,
                                     void *masks, void *stream)
{
    if (hp_ks == NULL || (n != 0 && (hp == NULL || base == NULL || masks == NULL)))
        return fail("%s", "chacha hp_mask: invalid arguments");
    if (n == 0)
        return 0;
    DeviceScope scope(hp_ks->device);
    hipStream_t s = (hipStream_t)stream;
    std::lock_guard<std::mutex> lk(hp_ks->mu);
    return chacha_launch_noted(hp_ks, s, "chacha hp_mask launch: %s", [&] {
        chacha_hp_kernel<<<aux_grid(n, hp_ks->ds->ncu), 256, 0, s>>>(hp_ks->d_keys, (u32)hp_ks->nkeys, hp, (const uint8_t *)base,
                                                                     (uint8_t *)masks, n, nullptr, 0);
    });
}

}  // extern "C"

// one record on host buffers: staged, sealed or opened by one launch on the stager's stream, copied back. The launch is
// one workgroup, or from CHACHA_SPREAD_MIN_SINGLE bytes a spread one of as many workgroups as the record's pieces need
// (its accumulators are a claim slot's, in device memory: atomics on the mapped staging buffer would cross the bus).
static int chacha_single(ptls_mi355x_chacha_keyset_t *ks, size_t key_idx, bool open, void *output, const ptls_mi355x_iovec_t *vec,
                         size_t incnt, size_t len, uint64_t seq, const void *aad, size_t aadlen, int *verified)
{
    if (check_single_args("chacha single", ks != NULL && key_idx < ks->nkeys, aad, aadlen, output, len) != 0)
        return -1;
    DeviceScope scope(ks->device);
    StageCall call(ks->ds);
    // staging: [0, 40) descriptor | AAD | input (open: with the tag) || output (seal: with the tag) | ok byte | done word
    const size_t aad_at = 64, in_at = aad_at + ((aadlen + 63) & ~(size_t)63), in_len = len + (open ? 16 : 0);
    const size_t out_at = in_at + ((in_len + 63) & ~(size_t)63), out_len = len + (open ? 0 : 16);
    const size_t ok_at = out_at + ((out_len + 63) & ~(size_t)63), flag_at = ok_at + 16;
    const u32 force_g = g_chacha_force_g.load(std::memory_order_relaxed), base_piece = chacha_spread_base_piece();
    const bool spread = len >= chacha_spread_min_len(CHACHA_SPREAD_MIN_SINGLE) && len <= PTLS_MI355X_MAX_RECORD_LEN &&
                        aadlen <= PTLS_MI355X_MAX_AAD_LEN && chacha_spread_allowed(force_g);
    unsigned nwg = 1;
    if (spread) {
        const u32 piece = chacha_spread_piece((u32)len, base_piece);
        nwg = chacha_spread_grid(ks->ds, ((len + piece - 1) / piece + CHACHA_WG / CHACHA_G_WIDE - 1) / (CHACHA_WG / CHACHA_G_WIDE));
    }
    if (call.acquire(flag_at + (((size_t)nwg * 4 + 15) & ~(size_t)15)) != 0)
        return -1;
    uint8_t *h = call.host();
    ptls_mi355x_record_t rec = {};
    rec.in_off = in_at, rec.out_off = out_at, rec.seq = seq, rec.aad_off = (u32)aad_at, rec.len = (u32)len;
    rec.key_idx = (u32)key_idx, rec.aad_len = (uint16_t)aadlen, rec.flags = (uint16_t)(aadlen >> 16);
    memcpy(h, &rec, sizeof(rec));
    if (aadlen != 0)
        memcpy(h + aad_at, aad, aadlen);
    gather_iovec(h + in_at, vec, incnt);
    h[ok_at] = 0;
    memset(h + flag_at, 0, (size_t)nwg * 4);
    call.clear_lo = in_at, call.clear_hi = ok_at;
    uint8_t *d = call.dev();
    const hipStream_t s = call.stream();
    const u32 token = next_done_token();
    const int ret = call.roundtrip(out_at, [&] {
        ChaChaArgs a = {};
        a.keys = ks->d_keys, a.nkeys = (u32)ks->nkeys, a.force_g = force_g;
        a.recs = (const ptls_mi355x_record_t *)d, a.nrecs = 1, a.in = d, a.aad = d, a.out = d, a.ok = d + ok_at;
        a.claim = nullptr;  // one record: nothing to claim (a claim slot only for a spread launch's accumulators)
        a.done_flag = (u32 *)(d + flag_at), a.done_token = token;
        std::lock_guard<std::mutex> lk(ks->mu);
        if (spread) {
            const unsigned *slot = ks->slots.get(s, ks->uses, [&](unsigned &i) { return i = (unsigned)ks->slots.v.size(), true; });
            ChaChaSpreadArgs sa = {};
            sa.a = a, sa.piece = base_piece, sa.min_len = 1;  // (the length was weighed above)
            if (slot == nullptr || (sa.acc = chacha_spread_scratch(ks, *slot, s)) == nullptr)
                return -1;
            return chacha_launch_noted(ks, s, "chacha single launch: %s", [&] { chacha_launch_spread(open, nwg, s, sa); });
        }
        return chacha_launch_noted(ks, s, "chacha single launch: %s", [&] { chacha_launch_kernel(open, 0, 1, s, a); });
    }, flag_at, nwg, token);
    if (ret != 0)
        return -1;
    if (open) {
        *verified = h[ok_at] == 1;
        if (*verified && len != 0)
            memcpy(output, h + out_at, len);  // a record that failed leaves the caller's output as it was
    } else {
        memcpy(output, h + out_at, len + 16);
    }
    return 0;
}

extern "C" {

int ptls_mi355x_chacha_encrypt(ptls_mi355x_chacha_keyset_t *ks, size_t key_idx, void *output, const void *input, size_t inlen,
                               uint64_t seq, const void *aad, size_t aadlen)
{
    const ptls_mi355x_iovec_t v = {input, inlen};
    if (output == NULL || (inlen != 0 && input == NULL))
        return fail("%s", "chacha encrypt: invalid arguments");
    return chacha_single(ks, key_idx, false, output, &v, 1, inlen, seq, aad, aadlen, NULL);
}

int ptls_mi355x_chacha_encrypt_v(ptls_mi355x_chacha_keyset_t *ks, size_t key_idx, void *output, const ptls_mi355x_iovec_t *input,
                                 size_t incnt, uint64_t seq, const void *aad, size_t aadlen)
{
    size_t len = 0;
    if (output == NULL || (incnt != 0 && input == NULL))
        return fail("%s", "chacha encrypt_v: invalid arguments");
    for (size_t i = 0; i < incnt; ++i) {
        if (input[i].len != 0 && input[i].base == NULL)
            return fail("%s", "chacha encrypt_v: invalid iovec");
        len += input[i].len;
    }
    return chacha_single(ks, key_idx, false, output, input, incnt, len, seq, aad, aadlen, NULL);
}

size_t ptls_mi355x_chacha_decrypt(ptls_mi355x_chacha_keyset_t *ks, size_t key_idx, void *output, const void *input, size_t inlen,
                                  uint64_t seq, const void *aad, size_t aadlen)
{
    if (inlen < 16 || input == NULL)
        return SIZE_MAX;
    int verified = 0;
    const ptls_mi355x_iovec_t v = {input, inlen};
    if (chacha_single(ks, key_idx, true, output, &v, 1, inlen - 16, seq, aad, aadlen, &verified) != 0)
        return SIZE_MAX;
    return verified ? inlen - 16 : SIZE_MAX;
}

int ptls_mi355x_chacha_hp_mask(ptls_mi355x_chacha_keyset_t *hp_ks, size_t key_idx, void *mask, const void *sample)
{
    if (hp_ks == NULL || key_idx >= hp_ks->nkeys || mask == NULL || sample == NULL)
        return fail("%s", "chacha hp_mask: invalid arguments");
    DeviceScope scope(hp_ks->device);
    StageCall call(hp_ks->ds);
    // staging: [0, 16) sample | [16, 32) entry || [64, 80) mask | [80, 84) done word
    if (call.acquire(96) != 0)
        return -1;
    uint8_t *h = call.host();
    const ptls_mi355x_hp_t e = {0, (u32)key_idx, 0};
    memcpy(h, sample, 16);
    memcpy(h + 16, &e, sizeof(e));
    memset(h + 80, 0, 4);
    uint8_t *d = call.dev();
    const hipStream_t s = call.stream();
    const u32 token = next_done_token();
    const int ret = call.roundtrip(64, [&] {
        std::lock_guard<std::mutex> lk(hp_ks->mu);
        return chacha_launch_noted(hp_ks, s, "chacha hp_mask launch: %s", [&] {
            chacha_hp_kernel<<<1, 256, 0, s>>>(hp_ks->d_keys, (u32)hp_ks->nkeys, (const ptls_mi355x_hp_t *)(d + 16), d, d + 64, 1,
                                               (u32 *)(d + 80), token);
        });
    }, 80, 1, token);
    if (ret != 0)
        return -1;
    memcpy(mask, h + 64, 16);
    return 0;
}

int ptls_mi355x_chacha_debug_poly1305(const void *key32, const void *msg, size_t len, void *tag16)
{
    if (key32 == NULL || tag16 == NULL || (len != 0 && msg == NULL))
        return fail("%s", "chacha debug_poly1305: invalid arguments");
    DeviceState *ds = current_device_state();
    if (ds == nullptr)
        return -1;
    StageCall call(ds);
    // staging: [0, 32) key | message || tag
    const size_t tag_at = 32 + ((len + 63) & ~(size_t)63);
    if (call.acquire(tag_at + 16) != 0)
        return -1;
    uint8_t *h = call.host();
    memcpy(h, key32, 32);
    if (len != 0)
        memcpy(h + 32, msg, len);
    uint8_t *d = call.dev();
    const hipStream_t s = call.stream();
    if (call.roundtrip(tag_at, [&] {
            chacha_poly1305_kernel<<<1, 64, 0, s>>>(d, d + 32, (u64)len, d + tag_at);
            HIP_TRY(hipGetLastError());
            return 0;
        }) != 0)
        return -1;
    memcpy(tag16, h + tag_at, 16);
    return 0;
}

int ptls_mi355x_chacha_debug_force(int group_lanes, int max_workgroups)
{
    if ((group_lanes != 0 && group_lanes != CHACHA_G_NARROW && group_lanes != CHACHA_G_WIDE) || max_workgroups < 0)
        return fail("%s", "chacha debug_force: group_lanes is 0, 4 or 16 and max_workgroups is not negative");
    g_chacha_force_g.store((u32)group_lanes, std::memory_order_relaxed);
    g_chacha_force_wgs.store((u32)max_workgroups, std::memory_order_relaxed);
    return 0;
}

int ptls_mi355x_chacha_debug_spread(int piece_bytes, int min_len, int force)
{
    if (piece_bytes < 0 || piece_bytes % 1024 != 0 || piece_bytes > (1 << 20) || min_len < 0)
        return fail("%s", "chacha debug_spread: piece_bytes is 0 or a multiple of 1024 up to 2^20 and min_len is not negative");
    g_chacha_spread_piece.store((u32)piece_bytes, std::memory_order_relaxed);
    g_chacha_spread_min.store((u32)min_len, std::memory_order_relaxed);
    g_chacha_spread_force.store(force != 0, std::memory_order_relaxed);
    return 0;
}

int ptls_mi355x_chacha_debug_spread_counters(uint64_t *out, int reset)
{
    if (out == NULL)
        return fail("%s", "chacha debug_spread_counters: invalid arguments");
    HIP_TRY(hipDeviceSynchronize());  // (test-only) every launch made so far has counted itself
    unsigned long long n[4] = {0, 0, 0, 0};
    HIP_TRY(hipMemcpyFromSymbol(n, HIP_SYMBOL(g_chacha_spread_stats), sizeof(n)));
    for (int i = 0; i < 4; ++i)
        out[i] = n[i], n[i] = 0;
    if (reset)
        HIP_TRY(hipMemcpyToSymbol(HIP_SYMBOL(g_chacha_spread_stats), n, sizeof(n)));
    return 0;
}

int ptls_mi355x_chacha_debug_spread_params(uint32_t *out)
{
    if (out == NULL)
        return fail("%s", "chacha debug_spread_params: invalid arguments");
    out[0] = CHACHA_SPREAD_MIN_BATCH, out[1] = CHACHA_SPREAD_MIN_SINGLE, out[2] = CHACHA_SPREAD_MAX_RECS, out[3] = CHACHA_SPREAD_PIECE;
    return 0;
}

int ptls_mi355x_chacha_debug_rpow(const void *r16, uint64_t e, void *out17)
{
    if (r16 == NULL || out17 == NULL)
        return fail("%s", "chacha debug_rpow: invalid arguments");
    DeviceState *ds = current_device_state();
    if (ds == nullptr)
        return -1;
    StageCall call(ds);
    // staging: [0, 16) r || [64, 81) the power
    if (call.acquire(96) != 0)
        return -1;
    uint8_t *h = call.host();
    memcpy(h, r16, 16);
    uint8_t *d = call.dev();
    const hipStream_t s = call.stream();
    if (call.roundtrip(64, [&] {
            chacha_rpow_kernel<<<1, 64, 0, s>>>(d, (u64)e, d + 64);
            HIP_TRY(hipGetLastError());
            return 0;
        }) != 0)
        return -1;
    memcpy(out17, h + 64, 17);
    return 0;
}

int ptls_mi355x_chacha_debug_counters(uint64_t *out, int reset)
{
    if (out == NULL)
        return fail("%s", "chacha debug_counters: invalid arguments");
    HIP_TRY(hipDeviceSynchronize());  // (test-only) every launch made so far has counted itself
    unsigned long long n[2] = {0, 0};
    HIP_TRY(hipMemcpyFromSymbol(n, HIP_SYMBOL(g_chacha_launches), sizeof(n)));
    out[0] = n[0], out[1] = n[1];
    if (reset) {
        n[0] = n[1] = 0;
        HIP_TRY(hipMemcpyToSymbol(HIP_SYMBOL(g_chacha_launches), n, sizeof(n)));
    }
    return 0;
}

}  // extern "C"

#endif  // PTLS_MI355X_CHACHA_HOST_H
