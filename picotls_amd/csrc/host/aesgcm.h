// picotls_amd/csrc/host/aesgcm.h -- host side of the AES-GCM engine: the keyset, the launches, the batch C ABI of
// include/picotls/mi355x.h and include/picotls/mi355x_quic.h, the per-record path and the debug hooks of include/picotls/mi355x_debug.h.
// Part of the single translation unit picotls_amd/csrc/aesgcm_engine.hip (included after host/runtime.h; not standalone).
#ifndef PTLS_MI355X_HOST_AESGCM_H
#define PTLS_MI355X_HOST_AESGCM_H

// Test and measurement counters (include/picotls/mi355x_debug.h): chunked-kernel launches per EXT instantiation (0..4),
// lockstep launches (5), span launches (6), record-per-lane launches (7) -- host side, counted where the launch is made
static std::atomic<uint64_t> g_launches[8];
#define COUNT_LAUNCH(i) (ENGINE_HOOKS ? g_launches[(i)].fetch_add(1, std::memory_order_relaxed) : 0)

// The instantiations of gcm_chunked_kernel<NR, OPEN, FRAME, true, EXT> (the CT argument is instantiated true only,
// launch_chunked_x), for NR 10 and 14: EXT 1 (a spread plan) serves unframed batches, EXT 2 (header-protection masks)
// unframed seals, EXT 0, 3, 4 and 5 every frame and direction -- but EXT 3 not QUIC packets (frame 3), whose long whole
// runs the serial kernel takes (launch_chunked). set_kernel_attrs enumerates the set through this predicate and
// launch_chunked_x asserts it, so whatever is launched has its dynamic LDS size set.
constexpr bool chunked_instance(int frame, bool open, int ext)
{
    return frame < 0 || frame > 3 || ext < 0 || ext > 5 ? false
           : ext == 1                                   ? frame == 0
           : ext == 2                                   ? frame == 0 && !open
           : ext == 3                                   ? frame != 3
                                                        : true;
}

// (deduced return types and a left fold: such a template is instantiated where it is named and a left fold from its
// first element, so set_kernel_attrs names the kernels in the order written -- which is their order in the code object)
template <int NR, bool OPEN, int FRAME, int EXT>
static auto chunked_attr()
{
    if constexpr (chunked_instance(FRAME, OPEN, EXT))
        HIP_TRY(hipFuncSetAttribute((const void *)gcm_chunked_kernel<NR, OPEN, FRAME, true, EXT>, hipFuncAttributeMaxDynamicSharedMemorySize,
                                    CLDS_ALLOC));
    return 0;
}

// the instances of EXT...: for each frame, for each of EXT..., for each key size, seal then open
template <int... EXT, size_t... I>
static auto chunked_attrs_at(std::index_sequence<I...>)
{
    constexpr int ext[] = {EXT...};
    constexpr size_t n = sizeof...(EXT);
    int ret = 0;
    (..., (ret = ret != 0 ? ret : chunked_attr<I / 2 % 2 == 0 ? 10 : 14, I % 2 != 0, (int)(I / (4 * n)), ext[I / 4 % n]>()));
    return ret;
}

template <int... EXT>
static auto chunked_attrs() { return chunked_attrs_at<EXT...>(std::make_index_sequence<4 * sizeof...(EXT) * 4>{}); }

static int set_kernel_attrs(void)
{
    const auto lds = [](size_t bytes, auto... kernel) {
        hipError_t e = hipSuccess;
        (..., (e = e != hipSuccess ? e : hipFuncSetAttribute((const void *)kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes)));
        return e != hipSuccess ? fail("hipFuncSetAttribute: %s", hipGetErrorString(e)) : 0;
    };
    // (chunked: the special forms of unframed batches, the W8 kernels with (round 6) their multi-key form, the plain one)
    const bool ok = lds(LDS_ALLOC, gcm_batch_kernel<10, false>, gcm_batch_kernel<10, true>, gcm_batch_kernel<14, false>,
                        gcm_batch_kernel<14, true>) == 0 &&
                    chunked_attrs<1>() == 0 && chunked_attrs<2>() == 0 && chunked_attrs<3, 4, 5>() == 0 && chunked_attrs<0>() == 0 &&
                    lds(LDS_AES_BYTES, ecb_kernel<10>, ecb_kernel<14>, hp_kernel<10>, hp_kernel<14>, quiclb_kernel<10>) == 0 &&
                    lds(LDS_AES_BYTES, quic_unmask_kernel<10>, quic_unmask_kernel<14>, quic_protect_kernel<10>,
                        quic_protect_kernel<14>) == 0 &&
                    lds(SPAN_LDS, gcm_span_kernel<10, false, true>, gcm_span_kernel<10, true, true>, gcm_span_kernel<14, false, true>,
                        gcm_span_kernel<14, true, true>) == 0 &&
                    lds(LANE_LDS_BYTES, gcm_lane_kernel<10, false, 0>, gcm_lane_kernel<10, true, 0>, gcm_lane_kernel<14, false, 0>,
                        gcm_lane_kernel<14, true, 0>, gcm_lane_kernel<10, false, 3>, gcm_lane_kernel<10, true, 3>,
                        gcm_lane_kernel<14, false, 3>, gcm_lane_kernel<14, true, 3>) == 0 &&
                    lds(LANE_LDS_BYTES, gcm_lane_kernel<10, false, 1>, gcm_lane_kernel<10, true, 1>, gcm_lane_kernel<14, false, 1>,
                        gcm_lane_kernel<14, true, 1>, gcm_lane_kernel<10, false, 2>, gcm_lane_kernel<10, true, 2>,
                        gcm_lane_kernel<14, false, 2>, gcm_lane_kernel<14, true, 2>) == 0;
    return ok ? 0 : -1;
}

#define W8_FLAG_STREAMS 8  // streams of a keyset with a W8 flag buffer of their own (w8_flags_locked)

struct st_ptls_mi355x_keyset_t {
    DeviceState *ds;
    int device;
    size_t nkeys, key_size;
    int nr;
    KeyEntry *d_keys;
    bool slot;  // d_keys is one entry of the device's slab (one-key keysets)
    KeyEntry *slab;  // ... that slab
    int schedule;
    bool lane_framed;                  // under RECORD_PER_LANE the TLS-framed calls and seal_batch_hp take the lane kernel too
    bool ct;                           // constant-time GHASH (ptls_mi355x_keyset_set_constant_time)
    hipEvent_t ready;                  // the last setup / update / set_iv of the entries
    std::atomic<bool> ready_seen;      // ... known to be complete: launches need not wait for it
    // a one-key keyset's setup waits for its first use and runs on that use's stream (no cross-stream wait for the
    // first seal of a context); until then the raw key stays here (cleared once launched)
    std::atomic<bool> pending;
    RawKey raw;
    std::vector<uint8_t> ivs;          // the static IVs (do_get_iv reads these; the device copy is what seals use)
    std::mutex mu;                     // launches from several threads: uses and the scratch below
    StreamUses uses;                   // per stream: after this keyset's last launch on it
    // Scratch lent to launches on any stream (host/runtime.h Scratch), each grown to the largest batch seen so far:
    Scratch group;   // ungrouped many-key batches (key_group_*): key counts, the record permutation, balance tiles
    Scratch spread;  // small batches with long records (spread_pieces): per-record counters (zero between launches),
                     // then the pieces' partials (spread_bytes)
    Scratch quic;    // QUIC packets (launch_quic): the descriptors the pre-pass writes for the batch kernel
    // W8 launch pairs (launch_chunked): one word per workgroup from the pair's first kernel to its second,
    // one buffer per stream (allocated on the stream's first pair; a stream orders its own pairs), so that pairs on
    // several streams run concurrently; at most W8_FLAG_STREAMS (StreamSlots)
    StreamSlots<Scratch, W8_FLAG_STREAMS> w8flags;
};

static int mark_ready(ptls_mi355x_keyset_t *ks, hipStream_t s);

// launches a pending one-key setup on `s` (the stream of the keyset's first use, or the maintenance stream); returns 1
// when it did (work on `s` is then ordered after it), 0 when there was none, -1 on failure
static int setup_now(ptls_mi355x_keyset_t *ks, hipStream_t s)
{
    if (!ks->pending.load(std::memory_order_acquire))
        return 0;
    std::lock_guard<std::mutex> lk(ks->mu);
    if (!ks->pending.load(std::memory_order_relaxed))
        return 0;
    LAUNCH_CLEAR();
    keyset_setup_one_kernel<<<1, 64, 0, s>>>(ks->raw, ks->d_keys);
    if (hipGetLastError() != hipSuccess)
        return fail("%s", "keyset setup launch failed");
    clear_memory(&ks->raw, sizeof(ks->raw));
    if (mark_ready(ks, s) != 0)
        return -1;
    ks->pending.store(false, std::memory_order_release);
    return 1;
}

// makes `s` wait for the keyset's last setup / update / set_iv, unless that is known to be complete
static int wait_ready(ptls_mi355x_keyset_t *ks, hipStream_t s)
{
    const int now = setup_now(ks, s);
    if (now != 0)
        return now < 0 ? -1 : 0;
    if (ks->ready_seen.load(std::memory_order_acquire))
        return 0;
    hipError_t q = hipEventQuery(ks->ready);
    if (q == hipSuccess) {
        ks->ready_seen.store(true, std::memory_order_release);
        return 0;
    }
    if (q != hipErrorNotReady)
        return fail("keyset setup failed: %s", hipGetErrorString(q));
    (void)hipGetLastError();  // (not an error: launches after this are checked with hipGetLastError)
    HIP_TRY(hipStreamWaitEvent(s, ks->ready, 0));
    return 0;
}

// orders the maintenance stream after every launch that used the keyset and after its last setup
static int maint_after_uses(ptls_mi355x_keyset_t *ks)
{
    if (setup_now(ks, ks->ds->maint) < 0)
        return -1;
    std::lock_guard<std::mutex> lk(ks->mu);
    if (ks->uses.order_after_all(ks->ds->maint) != 0)
        return -1;
    if (!ks->ready_seen.load(std::memory_order_acquire))
        HIP_TRY(hipStreamWaitEvent(ks->ds->maint, ks->ready, 0));
    return 0;
}

static int mark_ready(ptls_mi355x_keyset_t *ks, hipStream_t s)
{
    ks->ready_seen.store(false, std::memory_order_release);
    HIP_TRY(hipEventRecord(ks->ready, s));
    return 0;
}

static void keyset_destroy(ptls_mi355x_keyset_t *ks)
{
    DeviceState *ds = ks->ds;
    ks->uses.release(ds);
    event_put(ds, ks->ready);
    clear_memory(ks->ivs.data(), ks->ivs.size());
    clear_memory(&ks->raw, sizeof(ks->raw));
    delete ks;
}

extern "C" {

const char *ptls_mi355x_last_error(void) { return g_err; }

int ptls_mi355x_is_supported(void)
{
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n == 0)
        return 0;
    int dev = 0;
    hipDeviceProp_t prop;
    if (hipGetDevice(&dev) != hipSuccess || hipGetDeviceProperties(&prop, dev) != hipSuccess)
        return 0;
    return strncmp(prop.gcnArchName, "gfx950", 6) == 0;
}

ptls_mi355x_keyset_t *ptls_mi355x_keyset_new(const void *keys, const void *ivs, size_t nkeys, size_t key_size)
{
    if (keys == NULL || ivs == NULL || nkeys == 0 || (key_size != 16 && key_size != 32) || nkeys > (1u << 30)) {
        fail("%s", "ptls_mi355x_keyset_new: invalid arguments");
        return NULL;
    }
    DeviceState *ds = current_device_state();
    if (ds == nullptr)
        return NULL;
    ptls_mi355x_keyset_t *ks = new (std::nothrow) st_ptls_mi355x_keyset_t();
    if (ks == nullptr) {
        fail("%s", "out of memory");
        return NULL;
    }
    ks->ds = ds;
    ks->device = ds->device;
    ks->nkeys = nkeys, ks->key_size = key_size, ks->nr = key_size == 16 ? 10 : 14;
    ks->ct = ds->ct_default;
    ks->ready_seen.store(false);
    ks->pending.store(false);
    ks->ivs.assign((const uint8_t *)ivs, (const uint8_t *)ivs + nkeys * 12);
    if ((ks->ready = event_get(ds)) == nullptr) {
        fail("%s", "ptls_mi355x_keyset_new: event creation failed");
        delete ks;
        return NULL;
    }
    if (nkeys == 1) {
        // a picotls context: a slab entry, and the setup launch (the key in its arguments) deferred to the first use,
        // on that use's stream (setup_now)
        if ((ks->d_keys = slot_get(ds, &ks->slab)) == nullptr) {
            keyset_destroy(ks);
            return NULL;
        }
        ks->slot = true;
        memcpy(ks->raw.key, keys, key_size);
        memcpy(ks->raw.iv, ivs, 12);
        ks->raw.key_size = (u32)key_size;
        ks->pending.store(true, std::memory_order_release);
        return ks;
    }
    // many keys: entries and the raw key material in stream-ordered memory on the setup stream. The caller's arrays are
    // pageable host memory, so the call waits (for the setup stream only) until the copies have consumed them.
    uint8_t *d_raw = nullptr;
    const size_t raw_bytes = nkeys * (key_size + 12);
    free_after_maint(ds, nullptr);  // (entries of freed keysets whose clearing has run go back to the pool)
    bool ok = hipMallocAsync((void **)&ks->d_keys, nkeys * sizeof(KeyEntry), ds->setup) == hipSuccess &&
              hipMallocAsync((void **)&d_raw, raw_bytes, ds->setup) == hipSuccess &&
              hipMemcpyAsync(d_raw, keys, nkeys * key_size, hipMemcpyHostToDevice, ds->setup) == hipSuccess &&
              hipMemcpyAsync(d_raw + nkeys * key_size, ivs, nkeys * 12, hipMemcpyHostToDevice, ds->setup) == hipSuccess;
    if (ok) {
        LAUNCH_CLEAR();
        keyset_setup_kernel<<<(unsigned)((nkeys + 127) / 128), 128, 0, ds->setup>>>(d_raw, d_raw + nkeys * key_size, ks->d_keys,
                                                                                   (u32)nkeys, (u32)key_size);
        ok = hipGetLastError() == hipSuccess;
    }
    if (d_raw != nullptr) {
        (void)hipMemsetAsync(d_raw, 0, raw_bytes, ds->setup);
        (void)hipFreeAsync(d_raw, ds->setup);
    }
    if (ok)
        ok = mark_ready(ks, ds->setup) == 0 && hipStreamSynchronize(ds->setup) == hipSuccess;
    if (!ok) {
        if (ks->d_keys != nullptr)
            (void)hipFreeAsync(ks->d_keys, ds->setup);
        fail("%s", "ptls_mi355x_keyset_new: device setup failed");
        keyset_destroy(ks);
        return NULL;
    }
    return ks;
}

int ptls_mi355x_keyset_update(ptls_mi355x_keyset_t *ks, const uint32_t *key_idx, const void *keys, const void *ivs, size_t n)
{
    if (ks == NULL || (n != 0 && (key_idx == NULL || keys == NULL || ivs == NULL)))
        return fail("%s", "keyset_update: invalid arguments");
    if (check_update_indices("keyset_update", key_idx, n, ks->nkeys) != 0)
        return -1;
    if (n == 0)
        return 0;
    DeviceScope scope(ks->device);
    DeviceState *ds = ks->ds;
    // stream-ordered on the maintenance stream: after every launch already made with the old entries, before any made
    // after this call (they wait for `ready`)
    if (maint_after_uses(ks) != 0)
        return -1;
    uint8_t *d = NULL;
    const size_t kb = n * ks->key_size, ib = n * 12, sb = n * 4;
    HIP_TRY(hipMallocAsync((void **)&d, kb + ib + sb, ds->maint));
    int ret = -1;
    if (hipMemcpyAsync(d, keys, kb, hipMemcpyHostToDevice, ds->maint) == hipSuccess &&
        hipMemcpyAsync(d + kb, ivs, ib, hipMemcpyHostToDevice, ds->maint) == hipSuccess &&
        hipMemcpyAsync(d + kb + ib, key_idx, sb, hipMemcpyHostToDevice, ds->maint) == hipSuccess) {
        LAUNCH_CLEAR();
        keyset_setup_kernel<<<(unsigned)((n + 127) / 128), 128, 0, ds->maint>>>(d, d + kb, ks->d_keys, (u32)n, (u32)ks->key_size,
                                                                               (const u32 *)(d + kb + ib));
        if (hipGetLastError() == hipSuccess && mark_ready(ks, ds->maint) == 0)
            ret = 0;
    }
    (void)hipMemsetAsync(d, 0, kb + ib, ds->maint);
    (void)hipFreeAsync(d, ds->maint);
    // the caller's pageable arrays must have been consumed before returning
    if (hipStreamSynchronize(ds->maint) != hipSuccess)
        ret = -1;
    if (ret != 0)
        return fail("%s", "keyset_update: device setup failed");
    for (size_t i = 0; i < n; ++i)
        memcpy(ks->ivs.data() + (size_t)key_idx[i] * 12, (const uint8_t *)ivs + i * 12, 12);
    return 0;
}

void ptls_mi355x_keyset_free(ptls_mi355x_keyset_t *ks)
{
    if (ks == NULL)
        return;
    DeviceScope scope(ks->device);
    DeviceState *ds = ks->ds;
    ks->pending.store(false, std::memory_order_release);  // never used: its setup never ran (the raw key is cleared below)
    // key material is cleared (ptls_clear_memory, lib/fusion.c:1045) after the keyset's last launch, on the maintenance
    // stream; nothing here waits on the host
    const bool ordered = !ds->fault_order && maint_after_uses(ks) == 0;
    if (!ordered) {
        // the teardown cannot be ordered after the keyset's launches on the device: wait for each of them (the recorded
        // uses on every stream -- every launch that took scratch is among them -- and the setup) on the host before
        // clearing; if even that fails, keep the entries and the scratch as they are and never reuse them, rather than
        // clear them under a launch still reading them
        bool drained;
        {
            std::lock_guard<std::mutex> lk(ks->mu);
            drained = ks->uses.drain();
        }
        drained = hipEventSynchronize(ks->ready) == hipSuccess && drained;
        if (!drained) {
            keyset_destroy(ks);
            return;
        }
    }
    (void)hipMemsetAsync(ks->d_keys, 0, ks->nkeys * sizeof(KeyEntry), ds->maint);
    ks->group.release(ds, false);
    ks->spread.release(ds, false);
    ks->quic.release(ds, false);
    for (auto &f : ks->w8flags.v)
        f.second.release(ds, false);
    if (ks->slot) {
        // back to the pool once the clear has run (slot_get checks the event)
        hipEvent_t cleared = event_get(ds);
        if (cleared != nullptr && hipEventRecord(cleared, ds->maint) == hipSuccess) {
            std::lock_guard<std::mutex> lk(ds->mu);
            ds->pending.push_back({ks->d_keys, ks->slab, cleared});
        }
    } else {
        free_after_maint(ds, ks->d_keys);
    }
    keyset_destroy(ks);
}

#if ENGINE_PROFILE
int ptls_mi355x_debug_profile(unsigned long long *out, int reset)
{
    HIP_TRY(hipDeviceSynchronize());
    static unsigned long long rows[PROF_ROWS][PROF_SLOTS];
    HIP_TRY(hipMemcpyFromSymbol(rows, HIP_SYMBOL(g_prof), sizeof(g_prof)));
    for (int i = 0; i < PROF_SLOTS; ++i) {
        out[i] = 0;
        for (int r = 0; r < PROF_ROWS; ++r)
            out[i] += rows[r][i];
    }
    if (reset) {
        memset(rows, 0, sizeof(rows));
        HIP_TRY(hipMemcpyToSymbol(HIP_SYMBOL(g_prof), rows, sizeof(g_prof)));
    }
    return 0;
}
#endif

// ---- test and measurement hooks (include/picotls/mi355x_debug.h)

// reads (and with reset, zeroes in the same atomic exchange) the per-workgroup run counters, so that a launch finishing
// meanwhile is counted once, in this read or the next
__global__ void ext_runs_take_kernel(unsigned long long *out, int reset)
{
    for (u32 i = threadIdx.x; i < EXT_RUN_ROWS * 8; i += blockDim.x) {
        unsigned long long *c = &g_ext_runs[i / 8][i % 8];
        out[i] = reset ? atomicExch(c, 0ull) : __hip_atomic_load(c, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

int ptls_mi355x_debug_counters(uint64_t *out, int reset)
{
    if (out == NULL)
        return fail("%s", "debug_counters: invalid arguments");
    // (test-only) every launch made so far has finished, and counted its runs, before anything is read
    HIP_TRY(hipDeviceSynchronize());
    for (int i = 0; i < 8; ++i)
        out[i] = reset ? g_launches[i].exchange(0) : g_launches[i].load();
    std::vector<unsigned long long> rows((size_t)EXT_RUN_ROWS * 8);
    unsigned long long *d = nullptr;
    HIP_TRY(hipMalloc(&d, rows.size() * sizeof(rows[0])));
    LAUNCH_CLEAR();
    ext_runs_take_kernel<<<1, 256>>>(d, reset);
    hipError_t e = hipGetLastError();
    if (e == hipSuccess)
        e = hipMemcpy(rows.data(), d, rows.size() * sizeof(rows[0]), hipMemcpyDeviceToHost);
    (void)hipFree(d);
    if (e != hipSuccess)
        return fail("debug_counters: %s", hipGetErrorString(e));
    for (int i = 0; i < 8; ++i) {
        out[8 + i] = 0;
        for (int r = 0; r < EXT_RUN_ROWS; ++r)
            out[8 + i] += rows[(size_t)r * 8 + i];
    }
    return 0;
}

int ptls_mi355x_debug_kernel_clock(void *buf, unsigned cap)
{
    unsigned long long *b = (unsigned long long *)buf;
    const unsigned zero = 0, c = buf != NULL ? cap : 0;
    HIP_TRY(hipDeviceSynchronize());  // (test-only: no launch may be sampling while the buffer changes)
    HIP_TRY(hipMemcpyToSymbol(HIP_SYMBOL(g_kclock_n), &zero, sizeof(zero)));
    HIP_TRY(hipMemcpyToSymbol(HIP_SYMBOL(g_kclock_cap), &c, sizeof(c)));
    HIP_TRY(hipMemcpyToSymbol(HIP_SYMBOL(g_kclock_buf), &b, sizeof(b)));
    return 0;
}

int ptls_mi355x_debug_kernel_clock_count(void)
{
    unsigned n = 0;
    HIP_TRY(hipDeviceSynchronize());
    HIP_TRY(hipMemcpyFromSymbol(&n, HIP_SYMBOL(g_kclock_n), sizeof(n)));
    return (int)n;
}

int ptls_mi355x_debug_inject_error(void)
{
    // a handled-looking failure of the kind the per-record path meets (hipHostGetDevicePointer on memory HIP did not
    // allocate), deliberately NOT cleared: the thread's last error is left set, as a handled failure used to leave it
    static uint8_t pageable[64];
    void *p = nullptr;
    const hipError_t e = hipHostGetDevicePointer(&p, pageable, 0);
    return (int)(e != hipSuccess ? hipPeekAtLastError() : hipSuccess);
}

int ptls_mi355x_debug_clock_sample(void *out, void *stream)
{
    if (out == NULL)
        return fail("%s", "debug_clock_sample: invalid arguments");
    LAUNCH_CLEAR();
    clock_probe_kernel<<<1, 64, 0, (hipStream_t)stream>>>((unsigned long long *)out);
    HIP_TRY(hipGetLastError());
    return 0;
}

int ptls_mi355x_debug_wallclock_khz(void)
{
    int dev = 0, khz = 0;
    if (hipGetDevice(&dev) != hipSuccess || hipDeviceGetAttribute(&khz, hipDeviceAttributeWallClockRate, dev) != hipSuccess)
        return 0;
    return khz;
}

int ptls_mi355x_keyset_set_schedule(ptls_mi355x_keyset_t *ks, int schedule)
{
    if (ks == NULL || schedule < PTLS_MI355X_SCHEDULE_AUTO || schedule > PTLS_MI355X_SCHEDULE_RECORD_PER_LANE)
        return fail("%s", "set_schedule: invalid arguments");
    ks->schedule = schedule;
    return 0;
}

int ptls_mi355x_keyset_set_lane_framed(ptls_mi355x_keyset_t *ks, int on)
{
    if (ks == NULL)
        return fail("%s", "set_lane_framed: invalid arguments");
    ks->lane_framed = on != 0;
    return 0;
}

int ptls_mi355x_keyset_get_lane_framed(const ptls_mi355x_keyset_t *ks) { return ks != NULL && ks->lane_framed ? 1 : 0; }

int ptls_mi355x_keyset_set_constant_time(ptls_mi355x_keyset_t *ks, int on)
{
    if (ks == NULL)
        return fail("%s", "set_constant_time: invalid arguments");
    ks->ct = on != 0;
    return 0;
}

int ptls_mi355x_keyset_get_constant_time(const ptls_mi355x_keyset_t *ks) { return ks != NULL && ks->ct ? 1 : 0; }

size_t ptls_mi355x_keyset_size(const ptls_mi355x_keyset_t *ks) { return ks->nkeys; }
size_t ptls_mi355x_keyset_key_size(const ptls_mi355x_keyset_t *ks) { return ks->key_size; }
int ptls_mi355x_keyset_device(const ptls_mi355x_keyset_t *ks) { return ks->device; }

size_t ptls_mi355x_staging_bytes(void)
{
    size_t n = 0;
    for (int d = 0; d < MAX_DEVICES; ++d) {
        DeviceState *ds = g_devs[d].load(std::memory_order_acquire);
        if (ds == nullptr)
            continue;
        std::lock_guard<std::mutex> lk(ds->mu);
        n += ds->stage_idle + ds->stage_busy;
    }
    return n;
}

void ptls_mi355x_release_staging(void)
{
    for (int d = 0; d < MAX_DEVICES; ++d) {
        DeviceState *ds = g_devs[d].load(std::memory_order_acquire);
        if (ds == nullptr)
            continue;
        DeviceScope scope(d);
        release_idle_stagers(ds);
    }
}

int ptls_mi355x_keyset_get_iv(ptls_mi355x_keyset_t *ks, size_t key_idx, void *iv)
{
    if (ks == NULL || key_idx >= ks->nkeys || iv == NULL)
        return fail("%s", "get_iv: bad key index");
    memcpy(iv, ks->ivs.data() + key_idx * 12, 12);
    return 0;
}

int ptls_mi355x_keyset_set_iv(ptls_mi355x_keyset_t *ks, size_t key_idx, const void *iv)
{
    if (ks == NULL || key_idx >= ks->nkeys || iv == NULL)
        return fail("%s", "set_iv: bad key index");
    DeviceScope scope(ks->device);
    if (maint_after_uses(ks) != 0)
        return -1;
    u32 w[3];
    memcpy(w, iv, 12);
    LAUNCH_CLEAR();
    keyset_set_iv_kernel<<<1, 1, 0, ks->ds->maint>>>(ks->d_keys + key_idx, w[0], w[1], w[2]);
    HIP_TRY(hipGetLastError());
    if (mark_ready(ks, ks->ds->maint) != 0)
        return -1;
    memcpy(ks->ivs.data() + key_idx * 12, iv, 12);
    return 0;
}

}  // extern "C"

// Schedule choice (ptls_mi355x_keyset_set_schedule): AUTO = chunked. Its uniform runs take the whole-record path,
// which measured at or above the lockstep kernel on one-key uniform batches (929 vs 841 GiB/s on 16 KiB records,
// 784 vs 751 on 1200 B), and its chunked runs balance mixed lengths and short key runs.
static bool use_chunked(int schedule) { return schedule != PTLS_MI355X_SCHEDULE_LOCKSTEP; }
// ... and a constant-time keyset runs the chunked kernel on every schedule (the lockstep kernel is not constant-time).
// Three decisions test the schedule alone, so that a constant-time keyset set to the lockstep schedule runs the chunked
// kernel but neither spans a long record nor polls completion words (run_calls) nor combines its calls (combine_kind):
// they predate the constant-time default and are kept as they are, deliberately, not by oversight.
static bool runs_chunked(bool ct, int schedule) { return ct || use_chunked(schedule); }
static bool runs_chunked(const ptls_mi355x_keyset_t *ks) { return runs_chunked(ks->ct, ks->schedule); }
// The record-per-lane schedule (engine/lane_kernels.h) serves the unframed and QUIC-packet batch calls without
// header-protection masks and, on a keyset with lane_framed set (ptls_mi355x_keyset_set_lane_framed), the TLS 1.3 and
// TLS 1.2 framed calls (seal_batch_hp then makes two launches and passes no masks here); every other call of a keyset
// set to it runs as under AUTO (use_chunked is true for it). It is constant-time by layout, so a constant-time keyset
// takes it as set: it is not routed through runs_chunked.
static bool runs_lane(int schedule, bool lane_framed, int frame, bool hp)
{
    return schedule == PTLS_MI355X_SCHEDULE_RECORD_PER_LANE && (frame == 0 || frame == 3 || lane_framed) && !hp;
}

// Since the window-major segment ends the constant-time template argument changes no instruction of the chunked and
// span kernels: every keyset, constant-time or not, launches the CT instantiation, the only one in the
// code object
template <int NR, bool OPEN, int FRAME, int EXT = 0>
static void launch_chunked_x(unsigned grid, hipStream_t s, const BatchArgs &a)
{
    static_assert(chunked_instance(FRAME, OPEN, EXT), "no such gcm_chunked_kernel instantiation: set_kernel_attrs would not set its LDS size");
    COUNT_LAUNCH(EXT == 5 ? 4 : EXT);  // (the MK form of the serial W8 kernel counts as it)
    gcm_chunked_kernel<NR, OPEN, FRAME, true, EXT><<<grid, ENGINE_WG, CLDS_ALLOC, s>>>(a);
}

// the instantiation for the launch: unframed batches with a spread plan (EXT 1) or header-protection masks (EXT 2)
// have their own (gcm_chunked_kernel)
template <int NR, bool OPEN, int FRAME>
static void launch_chunked(unsigned grid, hipStream_t s, const BatchArgs &a)
{
    if constexpr (FRAME == 0) {
        if (a.spread) {
            launch_chunked_x<NR, OPEN, 0, 1>(grid, s, a);
            return;
        }
        if constexpr (!OPEN) {
            if (a.hp != nullptr) {
                launch_chunked_x<NR, false, 0, 2>(grid, s, a);
                return;
            }
        }
    }
    // The W8 kernels (the Horner step on an 8-bit H^8 table, ghash.h gmul8) for every run of an unframed or TLS-framed
    // batch: EXT 4 (segment ends by a serial lane Horner) takes all runs but those of long whole records, which EXT 3
    // (8-lane groups dealt records of one padding, its own priority bands, no code for cut runs) takes after it, each skipping the
    // other's runs and EXT 3 returning at once in the workgroups where EXT 4 saw none (BatchArgs::w8_split, w8_flags).
    // A batch of fewer than WHOLE_MIN_RECS records per workgroup in contiguous ranges holds no whole-record run: EXT 4
    // alone. Not for a per-record launch (it publishes completion words, and its 1-16-step units suit the 4-bit path),
    // nor a batch of fewer than W8_MIN_RECS records (the table build is not repaid). TLS 1.2 framing too (faster despite
    // EXT 4's 96-byte-per-lane seal spill, common.h).
    if (!a.one_inline && a.done_flag == nullptr && a.nrecs >= W8_MIN_RECS) {
        // (QUIC packets, FRAME 3: the serial kernel alone, for whole runs of long packets too; EXT 3 is not instantiated for them)
        const bool whole_possible = FRAME != 3 && (a.chunk != 0 || a.bounds != nullptr || (a.nrecs + grid - 1) / grid >= WHOLE_MIN_RECS);
        BatchArgs b = a;
        b.w8_split = whole_possible ? 2u : 1u;
        if (!whole_possible)
            b.w8_flags = nullptr;
        // (round 6) many-key batches take EXT 5: EXT 4 plus multi-key runs (gcm_kernels.h scan_mk); one-key batches
        // keep EXT 4, whose code the MK path would grow (small launches slowed by 5-14 % with it compiled in)
        if (a.multi_key)
            launch_chunked_x<NR, OPEN, FRAME, 5>(grid, s, b);
        else
            launch_chunked_x<NR, OPEN, FRAME, 4>(grid, s, b);
        if constexpr (FRAME != 3) {
            if (whole_possible)
                launch_chunked_x<NR, OPEN, FRAME, 3>(grid, s, b);
        }
        return;
    }
    launch_chunked_x<NR, OPEN, FRAME>(grid, s, a);
}

// Records per chunk of the chunked kernel's dealt-out assignment (BatchArgs::chunk), 0 for contiguous ranges. Each
// workgroup gets up to CHUNKS_PER_WG chunks spread over the batch, so that a batch ordered by record size (or by
// connections whose records differ in size) still shares its bytes evenly: 4M records of U[64 B, 16 KiB] sorted by
// length ran at 467 GiB/s seal+open with contiguous ranges against 802 in random order (bench.py, mixedsorted vs
// mixed1key). Chunks stay at least CHUNK_MIN_RECS records (whole-record runs need 128 and gain from more), and a
// batch too small for two such chunks per workgroup keeps contiguous ranges.
#ifndef CHUNKS_PER_WG
#define CHUNKS_PER_WG 8
#endif
#define CHUNK_MIN_RECS 256
// many-key batches: workgroup ranges balanced by weight (balance_*_kernel) from this many records (2 x 256 per workgroup)
#define BALANCE_MIN_RECS ((size_t)131072)
static u64 deal_chunk(u64 nrecs, u64 grid)
{
    for (u64 k = CHUNKS_PER_WG; k >= 2; k /= 2) {
        const u64 c = (nrecs + grid * k - 1) / (grid * k);
        if (c >= CHUNK_MIN_RECS)
            return c;
    }
    return 0;
}

// scratch of spread launches: per-record piece counters (SPREAD_MAX_RECS, zero between launches), then the pieces'
// partials: at most one piece per spare workgroup, or (records longer than 2^10 units x their share) 2^23 steps /
// SPREAD_UNIT_STEPS / 2^10 per record (PTLS_MI355X_MAX_RECORD_LEN)
#define SPREAD_MAX_RECS 255
#define SPREAD_CNT_BYTES ((size_t)256 * 4)

// Header-protection masks computed by the chunked seal launch itself (BatchArgs::hp; seal_batch_hp, encrypt_s)
struct HpLaunch {
    const ptls_mi355x_hp_t *hp;
    const KeyEntry *keys;
    u32 nkeys;
    int nr;
    uint8_t *masks;
};

// The GCM kernel launch of a batch (no key grouping, no keyset bookkeeping). The caller zero-initialises it and names
// what it has; of `a` that is keys, nkeys, recs, nrecs, in, aad (null: the AAD offsets are into `in`), out, ok, unit_log2
// and, where the launch uses them, grouped, perm, perm_on, bounds, done_flag, done_token, w8_flags. launch_gcm sets the rest.
struct GcmLaunch {
    BatchArgs a;
    hipStream_t stream;
    int nr, ncu, schedule;
    bool ct;    // the constant-time GHASH variant of the chunked kernel (the lockstep schedule is not offered in that mode)
    bool open;
    int frame;
    const HpLaunch *hp;               // header-protection masks in the same launch (chunked seal of unframed records only)
    const ptls_mi355x_record_t *one;  // the descriptor of a batch of one: the chunked kernel takes it from its arguments
    uint8_t *spread;                  // the keyset's spread scratch, for a batch that may use it (launch_batch)
    bool lane;                        // the record-per-lane kernel (launch_batch alone sets it: runs_lane)
};

static int launch_gcm(const GcmLaunch &g)
{
    BatchArgs a = g.a;
    const hipStream_t s = g.stream;
    const u64 nrecs = a.nrecs;
    const bool chunked = runs_chunked(g.ct, g.schedule);
    a.multi_key = a.nkeys > 1 ? 1u : 0u;
    if (g.lane) {
        // one workgroup per CU, each walking tiles of LANE_WG records (no key runs, no scratch)
        if (a.aad == NULL)
            a.aad = a.in;
        const u64 tiles = (nrecs + LANE_WG - 1) / LANE_WG;
        const unsigned lgrid = (unsigned)(tiles < (u64)g.ncu ? tiles : (u64)g.ncu);
        with_nr_open(g.nr, g.open, [&](auto NR, auto OPEN) {
            COUNT_LAUNCH(7);
            if (g.frame == 3)
                gcm_lane_kernel<NR, OPEN, 3><<<lgrid, LANE_WG, LANE_LDS_BYTES, s>>>(a);
            else if (g.frame == 2)
                gcm_lane_kernel<NR, OPEN, 2><<<lgrid, LANE_WG, LANE_LDS_BYTES, s>>>(a);
            else if (g.frame == 1)
                gcm_lane_kernel<NR, OPEN, 1><<<lgrid, LANE_WG, LANE_LDS_BYTES, s>>>(a);
            else
                gcm_lane_kernel<NR, OPEN, 0><<<lgrid, LANE_WG, LANE_LDS_BYTES, s>>>(a);
        });
        HIP_TRY(hipGetLastError());
        return 0;
    }
    if (g.hp != nullptr) {
        if (g.open || g.frame != 0 || !chunked)
            return fail("%s", "launch_gcm: header-protection masks need the chunked seal of unframed records");
        a.hp = g.hp->hp, a.hp_keys = g.hp->keys, a.hp_nkeys = g.hp->nkeys, a.hp_nr = (u32)g.hp->nr, a.masks = g.hp->masks;
    }
    if (g.one != nullptr && nrecs == 1)
        a.one_inline = 1, a.one = *g.one;
    if (a.aad == NULL)
        a.aad = a.in;
    // one persistent workgroup per CU. A batch with fewer records than CUs takes one workgroup per record, or (spread,
    // an unframed batch: spread_pieces) one per CU, the workgroups beyond the records sharing its long records
    u64 grid = (u64)g.ncu;
    if (g.spread != nullptr && g.frame == 0 && nrecs >= 2 && nrecs < (u64)g.ncu && nrecs <= SPREAD_MAX_RECS && g.hp == nullptr &&
        g.one == nullptr && chunked) {
        a.spread = 1;
        a.spread_cnt = (u32 *)g.spread;
        a.spread_part = (u32x4 *)(g.spread + SPREAD_CNT_BYTES);
    }
    if (grid > nrecs && !a.spread)
        grid = nrecs;
    if (grid < 1)
        grid = 1;
    a.chunk = deal_chunk(nrecs, grid);
    with_nr_open(g.nr, g.open, [&](auto NR, auto OPEN) {
        if (g.frame == 1)
            launch_chunked<NR, OPEN, 1>((unsigned)grid, s, a);
        else if (g.frame == 2)
            launch_chunked<NR, OPEN, 2>((unsigned)grid, s, a);
        else if (g.frame == 3)
            launch_chunked<NR, OPEN, 3>((unsigned)grid, s, a);
        else if (chunked)
            launch_chunked<NR, OPEN, 0>((unsigned)grid, s, a);
        else {
            COUNT_LAUNCH(5);
            gcm_batch_kernel<NR, OPEN><<<(unsigned)grid, ENGINE_WG, LDS_ALLOC, s>>>(a);
        }
    });
    HIP_TRY(hipGetLastError());
    return 0;
}

// One long record (descriptor g.one, key entry g.a.keys) over many workgroups (span_kernels.h): `units` 16-step units
// in spans of 2^e, their partials at `part` (nspans x 16 B, device-addressable), then the combine launch, which writes
// the tag or ok[0] and sets done_flag[0] when given.
static int launch_span(const GcmLaunch &g, u32 units, u32 e, u32 nspans, void *part)
{
    BatchArgs a = {g.a.keys, nullptr, 1, g.a.in, g.a.aad, g.a.out, g.a.ok, 0u, 1u, CHUNK_LOG2, nullptr, nullptr, nullptr, 1u, *g.one,
                   g.a.done_flag, 0, nullptr};
    a.done_token = g.a.done_token;
    with_nr_open(g.nr, g.open, [&](auto NR, auto OPEN) {
        COUNT_LAUNCH(6);  // (the CT instantiation for every keyset, as launch_chunked_x)
        gcm_span_kernel<NR, OPEN, true><<<nspans, ENGINE_WG, SPAN_LDS, g.stream>>>(a, 1u << e, units, (u32x4 *)part);
    });
    HIP_TRY(hipGetLastError());
    with_bool(g.open, [&](auto OPEN) {
        span_combine_kernel<OPEN><<<1, 256, GHASH_TABLE_BYTES + 16 * 257, g.stream>>>(a, nspans, e, (const u32x4 *)part);
    });
    HIP_TRY(hipGetLastError());
    return 0;
}

// (pieces of a record: at most its units / 2^10 + 1, 2^23 / SPREAD_UNIT_STEPS / 2^10 + 1 for the longest record)
// Sized for the batch's records (16 B x (CUs + 1025 pieces per record), 164 KiB for 10 records instead
// of 4.2 MB for the largest batch)
static size_t spread_bytes(int ncu, size_t nrecs)
{
    return SPREAD_CNT_BYTES + 16 * ((size_t)ncu + nrecs * (8192 / SPREAD_UNIT_STEPS + 1));
}

static bool spread_eligible(const ptls_mi355x_keyset_t *ks, size_t nrecs, int frame)
{
    return frame == 0 && nrecs >= 2 && nrecs < (size_t)ks->ds->ncu && nrecs <= SPREAD_MAX_RECS && runs_chunked(ks);
}

// a batch that may launch the W8 pair (launch_chunked): chunked, W8_MIN_RECS records
static bool w8_eligible(const ptls_mi355x_keyset_t *ks, size_t nrecs) { return nrecs >= W8_MIN_RECS && runs_chunked(ks); }

// the keyset's W8 flag words for a launch on `s`: the stream's own buffer (every word is written by the pair's first
// kernel before its second reads it), allocated in stream order on the stream's first pair, or taken over (StreamSlots).
// nullptr on failure: the pair then runs without them (EXT 3 scans every run). The caller holds ks->mu from here
// through the launch and the use event recorded after it (launch_batch). (A takeover waits twice for the stream that
// held the buffer, once for the slot and once for the block: the same event.)
static u32 *w8_flags_locked(ptls_mi355x_keyset_t *ks, hipStream_t s)
{
    Scratch *f = ks->w8flags.get(s, ks->uses, [](Scratch &) { return true; });
    if (f == nullptr)
        (void)hipGetLastError();
    return f != nullptr ? (u32 *)f->take(ks->ds, ks->uses, s, 4 * W8_FLAG_WORDS * (size_t)ks->ds->ncu) : nullptr;
}

// A batch call on a keyset: waits for the keyset's setup, groups an ungrouped many-key batch by key on the device, launches,
// and records the use (teardown and rekey are ordered after it).
static int launch_batch(ptls_mi355x_keyset_t *ks, bool open, const ptls_mi355x_record_t *recs, size_t nrecs, const void *in,
                        const void *aad, void *out, uint8_t *ok, void *stream, int frame = 0, const HpLaunch *hpl = nullptr,
                        std::unique_lock<std::mutex> *held = nullptr)
{
    if (ks == NULL || (nrecs != 0 && (recs == NULL || in == NULL || out == NULL || (open && ok == NULL))))
        return fail("%s", "batch: invalid arguments");
    if (nrecs == 0)
        return 0;
    DeviceScope scope(ks->device);
    hipStream_t s = (hipStream_t)stream;
    if (wait_ready(ks, s) != 0)
        return -1;
    LAUNCH_CLEAR();  // (the grouping kernels and launch_gcm's launch are checked after this)
    // ungrouped many-key batches: group the records by key on the device first (see key_hist_kernel)
    // (the record-per-lane schedule takes records in any key order: no grouping, no keyset scratch, ks->mu not taken for any)
    const bool lane = runs_lane(ks->schedule, ks->lane_framed, frame, hpl != nullptr);
    const bool group = !lane && use_chunked(ks->schedule) && ks->nkeys > 1 && ks->nkeys <= KEY_GROUP_MAX_KEYS && nrecs > 1 &&
                       nrecs <= 0xffffffffu;
    // the keyset's scratch (spread pieces, W8 flags, key grouping) is shared by its launches on every stream: ks->mu is
    // held from taking it (Scratch::take) through the launch and the use event after it. That event is
    // recorded whether or not the launch succeeded (launch_and_note), so it stands behind the scratch's last user for the
    // next stream that takes it, for a regrow and for teardown: the scratch needs no event of its own.
    // (launch_quic holds it already, around its own launches before and after this one: `held`, which stays locked)
    std::unique_lock<std::mutex> own(ks->mu, std::defer_lock);
    std::unique_lock<std::mutex> &lk = held != nullptr ? *held : own;
    GcmLaunch g = {};
    g.a.keys = ks->d_keys, g.a.nkeys = (u32)ks->nkeys, g.a.recs = recs, g.a.nrecs = nrecs, g.a.unit_log2 = CHUNK_LOG2;
    g.a.in = (const uint8_t *)in, g.a.aad = (const uint8_t *)aad, g.a.out = (uint8_t *)out, g.a.ok = ok;
    g.stream = s, g.nr = ks->nr, g.ncu = ks->ds->ncu, g.schedule = ks->schedule, g.ct = ks->ct, g.open = open, g.frame = frame, g.hp = hpl;
    g.lane = lane;
    // small batches with long records: the spread scratch, its counters zeroed when allocated (without it, the launch
    // runs unspread)
    if (!lane && hpl == nullptr && spread_eligible(ks, nrecs, frame)) {
        if (!lk.owns_lock())
            lk.lock();
        g.spread = (uint8_t *)ks->spread.take(ks->ds, ks->uses, s, spread_bytes(ks->ds->ncu, nrecs), SPREAD_CNT_BYTES);
    } else if (!lane && hpl == nullptr && w8_eligible(ks, nrecs)) {  // (a spread launch never takes the W8 pair)
        if (!lk.owns_lock())
            lk.lock();
        g.a.w8_flags = w8_flags_locked(ks, s);
    }
    if (group) {
        if (!lk.owns_lock())
            lk.lock();
        // scratch: ctl[2] | counts[nkeys + 1] | perm[n] | (8-byte aligned) grouped descriptors[n] | balance tiles | bounds
        const bool balance = nrecs >= BALANCE_MIN_RECS;
        const size_t ntiles = (nrecs + BALANCE_TILE - 1) / BALANCE_TILE, ncu = (size_t)ks->ds->ncu;
        const size_t gwords = ((2 + ks->nkeys + 1 + nrecs + 1) & ~(size_t)1) + nrecs * (sizeof(ptls_mi355x_record_t) / 4);
        const size_t twords = balance ? (ntiles + 1) & ~(size_t)1 : 0, bwords = balance ? 2 * (ncu + 1) : 0;
        const size_t nb = ks->nkeys + 1, words = gwords + twords + bwords;
        u32 *ctl = (u32 *)ks->group.take(ks->ds, ks->uses, s, words * 4);
        if (ctl == nullptr)
            return -1;
        u32 *cnt = ctl + 2, *perm = cnt + nb;
        HIP_TRY(hipMemsetAsync(ctl, 0, (2 + nb) * 4, s));
        const unsigned gh = (unsigned)min((nrecs + 255) / 256, (size_t)ks->ds->ncu * 8);
        key_changes_kernel<<<(unsigned)min((nrecs + 255) / 256, (size_t)ks->ds->ncu * KEY_CHANGES_WG_PER_CU), 256, 0, s>>>(recs, nrecs, ctl);
        key_hist_kernel<<<gh, 256, 0, s>>>(recs, nrecs, (u32)ks->nkeys, cnt, ctl);
        key_scan_kernel<<<1, 1024, 0, s>>>(cnt, (u32)nb, nrecs, ctl);
        ptls_mi355x_record_t *grouped = (ptls_mi355x_record_t *)(ctl + ((2 + nb + nrecs + 1) & ~(size_t)1));
        key_scatter_kernel<<<gh, 256, 0, s>>>(recs, nrecs, (u32)ks->nkeys, cnt, perm, grouped, ctl);
        u64 *bounds = nullptr;
        if (balance && use_chunked(ks->schedule)) {  // workgroup ranges of equal work (balance_bounds_kernel)
            u32 *tiles = ctl + gwords;
            bounds = (u64 *)(ctl + gwords + twords);
            const u32 grid = (u32)(ncu < nrecs ? ncu : nrecs);
            balance_tiles_kernel<<<(unsigned)min((ntiles + 3) / 4, ncu * 8), 256, 0, s>>>(recs, grouped, ctl + 1, nrecs, (u32)frame, tiles);
            balance_bounds_kernel<<<1, 1024, 0, s>>>(tiles, nrecs, grid, bounds);
        }
        g.a.grouped = grouped, g.a.perm = perm, g.a.perm_on = ctl + 1, g.a.bounds = bounds;
    }
    return launch_and_note(ks->uses, ks->ds, s, [&] {
        const int ret = launch_gcm(g);
        if (!lk.owns_lock())
            lk.lock();  // (a launch that took no scratch ran unlocked; the use is recorded under ks->mu)
        return ret;
    });
}

static int launch_ecb(const KeyEntry *keys, u32 nkeys, int nr, int ncu, const uint32_t *key_idx, const void *in, void *out,
                      size_t nblocks, hipStream_t s)
{
    LAUNCH_CLEAR();
    with_nr(nr, [&](auto NR) {
        ecb_kernel<NR><<<aux_grid(nblocks, ncu), 256, LDS_AES_BYTES, s>>>(keys, nkeys, key_idx, (const uint8_t *)in, (uint8_t *)out,
                                                                          nblocks);
    });
    HIP_TRY(hipGetLastError());
    return 0;
}

static int launch_hp(const KeyEntry *keys, u32 nkeys, int nr, int ncu, const ptls_mi355x_hp_t *hp, size_t n, const void *base,
                     void *masks, hipStream_t s, u32 *done_flag = nullptr, u32 done_token = 0)
{
    LAUNCH_CLEAR();
    with_nr(nr, [&](auto NR) {
        hp_kernel<NR><<<aux_grid(n, ncu), 256, LDS_AES_BYTES, s>>>(keys, nkeys, hp, (const uint8_t *)base, (uint8_t *)masks, n, done_flag,
                                                                    done_token);
    });
    HIP_TRY(hipGetLastError());
    return 0;
}

// QUIC packets (ptls_mi355x_seal_quic_packets / ptls_mi355x_open_quic_packets): the pre-pass, the FRAME 3 batch on the
// descriptors it wrote, the finish kernel (aux_kernels.h), all on `stream` with no host work between them. The
// descriptors live in ks's scratch (Scratch quic), so ks->mu is held from taking it through the last launch and the use event
// after it. The launches read both keysets: PairLock and launch_and_note_both (host/runtime.h).
static int launch_quic(ptls_mi355x_keyset_t *ks, ptls_mi355x_keyset_t *hp_ks, bool open, const ptls_mi355x_record_t *recs,
                       size_t nrecs, const void *in, void *out, uint8_t *ok, ptls_mi355x_quic_result_t *results, void *stream)
{
    if (check_quic_args("quic packets", ks, hp_ks, open, recs, nrecs, in, out, ok, results) != 0)
        return -1;
    if (nrecs == 0)
        return 0;
    DeviceScope scope(ks->device);
    hipStream_t s = (hipStream_t)stream;
    if (wait_ready(ks, s) != 0 || (hp_ks != ks && wait_ready(hp_ks, s) != 0))
        return -1;
    PairLock<ptls_mi355x_keyset_t> locks(ks, hp_ks);
    ptls_mi355x_record_t *desc = (ptls_mi355x_record_t *)ks->quic.take(ks->ds, ks->uses, s, nrecs * sizeof(ptls_mi355x_record_t));
    if (desc == nullptr)
        return -1;
    const unsigned grid = aux_grid(nrecs, ks->ds->ncu);
    // (the kernels with the AES tables in LDS: two workgroups of QUIC_AUX_WG threads a CU)
    const unsigned lgrid = (unsigned)min((u64)(nrecs + QUIC_AUX_WG - 1) / QUIC_AUX_WG, (u64)ks->ds->ncu * 2);
    return launch_and_note_both(ks, hp_ks, s, [&] {
        LAUNCH_CLEAR();
        if (open)
            with_nr(hp_ks->nr, [&](auto NR) {
                quic_unmask_kernel<NR><<<lgrid, QUIC_AUX_WG, LDS_AES_BYTES, s>>>(hp_ks->d_keys, (u32)hp_ks->nkeys, (u32)ks->nkeys, recs, nrecs,
                                                                       (const uint8_t *)in, (uint8_t *)out, results, desc);
            });
        else
            quic_seal_check_kernel<<<grid, 256, 0, s>>>((u32)hp_ks->nkeys, (u32)ks->nkeys, recs, nrecs, (const uint8_t *)in, desc);
        HIP_TRY(hipGetLastError());
        if (launch_batch(ks, open, desc, nrecs, in, NULL, out, ok, stream, 3, nullptr, &locks.ks_lock) != 0)
            return -1;
        LAUNCH_CLEAR();
        if (open)
            quic_status_kernel<<<grid, 256, 0, s>>>(ok, results, nrecs);
        else
            with_nr(hp_ks->nr, [&](auto NR) {
                quic_protect_kernel<NR><<<lgrid, QUIC_AUX_WG, LDS_AES_BYTES, s>>>(hp_ks->d_keys, desc, nrecs, (const uint8_t *)in, (uint8_t *)out);
            });
        HIP_TRY(hipGetLastError());
        return 0;
    });
}

extern "C" {

int ptls_mi355x_seal_quic_packets(ptls_mi355x_keyset_t *ks, ptls_mi355x_keyset_t *hp_ks, const ptls_mi355x_record_t *recs,
                                  size_t nrecs, const void *in, void *out, void *stream)
{
    return launch_quic(ks, hp_ks, false, recs, nrecs, in, out, NULL, NULL, stream);
}

int ptls_mi355x_open_quic_packets(ptls_mi355x_keyset_t *ks, ptls_mi355x_keyset_t *hp_ks, const ptls_mi355x_record_t *recs,
                                  size_t nrecs, const void *in, void *out, uint8_t *ok, ptls_mi355x_quic_result_t *results,
                                  void *stream)
{
    return launch_quic(ks, hp_ks, true, recs, nrecs, in, out, ok, results, stream);
}

int ptls_mi355x_seal_batch(ptls_mi355x_keyset_t *ks, const ptls_mi355x_record_t *recs, size_t nrecs, const void *in,
                           const void *aad, void *out, void *stream)
{
    return launch_batch(ks, false, recs, nrecs, in, aad, out, NULL, stream);
}

int ptls_mi355x_open_batch(ptls_mi355x_keyset_t *ks, const ptls_mi355x_record_t *recs, size_t nrecs, const void *in,
                           const void *aad, void *out, uint8_t *ok, void *stream)
{
    return launch_batch(ks, true, recs, nrecs, in, aad, out, ok, stream);
}

int ptls_mi355x_ecb_batch(ptls_mi355x_keyset_t *ks, const uint32_t *key_idx, const void *in, void *out, size_t nblocks,
                          void *stream)
{
    if (ks == NULL || (nblocks != 0 && (in == NULL || out == NULL)))
        return fail("%s", "ecb: invalid arguments");
    if (nblocks == 0)
        return 0;
    DeviceScope scope(ks->device);
    hipStream_t s = (hipStream_t)stream;
    if (wait_ready(ks, s) != 0 || launch_ecb(ks->d_keys, (u32)ks->nkeys, ks->nr, ks->ds->ncu, key_idx, in, out, nblocks, s) != 0)
        return -1;
    std::lock_guard<std::mutex> lk(ks->mu);
    return ks->uses.note(ks->ds, s);
}

int ptls_mi355x_seal_tls_records(ptls_mi355x_keyset_t *ks, const ptls_mi355x_record_t *recs, size_t nrecs, const void *in,
                                 void *out, void *stream)
{
    return launch_batch(ks, false, recs, nrecs, in, NULL, out, NULL, stream, 1);
}

int ptls_mi355x_open_tls_records(ptls_mi355x_keyset_t *ks, const ptls_mi355x_record_t *recs, size_t nrecs, const void *in,
                                 void *out, uint8_t *ok, ptls_mi355x_tls_result_t *results, void *stream)
{
    if (launch_batch(ks, true, recs, nrecs, in, NULL, out, ok, stream, 1) != 0)
        return -1;
    if (nrecs == 0)
        return 0;
    DeviceScope scope(ks->device);
    LAUNCH_CLEAR();
    tls_unpad_kernel<<<aux_grid(nrecs, ks->ds->ncu), 256, 0, (hipStream_t)stream>>>(recs, nrecs, (const uint8_t *)in,
                                                                                     (const uint8_t *)out, ok, results);
    HIP_TRY(hipGetLastError());
    return 0;
}

int ptls_mi355x_seal_tls12_records(ptls_mi355x_keyset_t *ks, const ptls_mi355x_record_t *recs, size_t nrecs, const void *in,
                                   void *out, void *stream)
{
    return launch_batch(ks, false, recs, nrecs, in, NULL, out, NULL, stream, 2);
}

int ptls_mi355x_open_tls12_records(ptls_mi355x_keyset_t *ks, const ptls_mi355x_record_t *recs, size_t nrecs, const void *in,
                                   void *out, uint8_t *ok, ptls_mi355x_tls_result_t *results, void *stream)
{
    if (launch_batch(ks, true, recs, nrecs, in, NULL, out, ok, stream, 2) != 0)
        return -1;
    if (nrecs == 0)
        return 0;
    DeviceScope scope(ks->device);
    LAUNCH_CLEAR();
    tls12_check_kernel<<<aux_grid(nrecs, ks->ds->ncu), 256, 0, (hipStream_t)stream>>>(recs, nrecs, (const uint8_t *)in, ok,
                                                                                       results);
    HIP_TRY(hipGetLastError());
    return 0;
}

int ptls_mi355x_hp_mask_batch(ptls_mi355x_keyset_t *hp_ks, const ptls_mi355x_hp_t *hp, size_t n, const void *base,
                              void *masks, void *stream)
{
    if (hp_ks == NULL || (n != 0 && (hp == NULL || base == NULL || masks == NULL)))
        return fail("%s", "hp_mask: invalid arguments");
    if (n == 0)
        return 0;
    DeviceScope scope(hp_ks->device);
    hipStream_t s = (hipStream_t)stream;
    if (wait_ready(hp_ks, s) != 0 || launch_hp(hp_ks->d_keys, (u32)hp_ks->nkeys, hp_ks->nr, hp_ks->ds->ncu, hp, n, base, masks, s) != 0)
        return -1;
    std::lock_guard<std::mutex> lk(hp_ks->mu);
    return hp_ks->uses.note(hp_ks->ds, s);
}

int ptls_mi355x_seal_batch_hp(ptls_mi355x_keyset_t *ks, const ptls_mi355x_record_t *recs, size_t nrecs, const void *in,
                              const void *aad, void *out, ptls_mi355x_keyset_t *hp_ks, const ptls_mi355x_hp_t *hp,
                              void *masks, void *stream)
{
    if (ks == NULL || hp_ks == NULL || (nrecs != 0 && (hp == NULL || masks == NULL)))
        return fail("%s", "seal_batch_hp: invalid arguments");
    if (hp_ks->device != ks->device)
        return fail("%s", "seal_batch_hp: the keysets are on different devices");
    if (nrecs == 0)
        return 0;
    // the lockstep schedule, or the record-per-lane one on a keyset with lane_framed set: the seal, then the masks (a
    // second launch on the stream, which reads the sealed bytes wherever the sample lies; each call records its keyset's use)
    if (!runs_chunked(ks) || (ks->schedule == PTLS_MI355X_SCHEDULE_RECORD_PER_LANE && ks->lane_framed)) {
        if (launch_batch(ks, false, recs, nrecs, in, aad, out, NULL, stream) != 0)
            return -1;
        return ptls_mi355x_hp_mask_batch(hp_ks, hp, nrecs, out, masks, stream);
    }
    // one launch: the chunked seal computes each run's masks after sealing it (hp_masks_pass)
    DeviceScope scope(ks->device);
    if (wait_ready(hp_ks, (hipStream_t)stream) != 0)
        return -1;
    const HpLaunch hpl = {hp, hp_ks->d_keys, (u32)hp_ks->nkeys, hp_ks->nr, (uint8_t *)masks};
    if (launch_batch(ks, false, recs, nrecs, in, aad, out, NULL, stream, 0, &hpl) != 0)
        return -1;
    std::lock_guard<std::mutex> lk(hp_ks->mu);
    return hp_ks->uses.note(hp_ks->ds, (hipStream_t)stream);
}

int ptls_mi355x_quiclb_batch(ptls_mi355x_keyset_t *ks, const ptls_mi355x_cid_t *cids, size_t n, const void *in, void *out,
                             void *stream)
{
    if (ks == NULL || (n != 0 && (cids == NULL || in == NULL || out == NULL)))
        return fail("%s", "quiclb: invalid arguments");
    if (ks->key_size != 16)
        return fail("%s", "quiclb: the QUIC-LB cipher is keyed with AES-128 (PTLS_QUICLB_KEY_SIZE)");
    if (n == 0)
        return 0;
    DeviceScope scope(ks->device);
    hipStream_t s = (hipStream_t)stream;
    if (wait_ready(ks, s) != 0)
        return -1;
    LAUNCH_CLEAR();
    quiclb_kernel<10><<<aux_grid(n, ks->ds->ncu), 256, LDS_AES_BYTES, s>>>(ks->d_keys, (u32)ks->nkeys, cids, (const uint8_t *)in,
                                                                            (uint8_t *)out, n);
    HIP_TRY(hipGetLastError());
    std::lock_guard<std::mutex> lk(ks->mu);
    return ks->uses.note(ks->ds, s);
}

}  // extern "C"

#ifndef SPAN_MIN_BYTES
#define SPAN_MIN_BYTES ((size_t)262144)  // a lone record from this length runs over many workgroups (launch_span)
#endif
#define PERREC_FLAG_MAX_BYTES ((size_t)1 << 20)  // staged bytes of a call that polls (larger ones wait for the stream)

// after a synchronous call on `ks` completed on a stager stream, its setup is complete too
static void seen_ready(ptls_mi355x_keyset_t *ks) { ks->ready_seen.store(true, std::memory_order_release); }

// ---- per-record calls, combined across threads
//
// picotls' per-record calls are synchronous, so one thread's records can never share a launch -- but the calls of
// several threads can. A call of a one-key keyset (a picotls context) goes to its device's combiner for its kind (seal
// or open, AES-128 or -256, constant-time or not, header-protection key size): when fewer than `combine` launches of
// that kind are in flight it takes every queued call, itself included, into one batch (flat combining); otherwise it
// queues and waits until a batch that took it completes, or until a launch slot frees and it can take the queue
// itself. A lone caller thus launches at once, as before, while N threads calling together share launches instead of
// queueing theirs on the device's few hardware queues (tools/mt_records.py). The entries of one-key keysets live in
// per-device slabs, so a combined batch addresses them as key indices from the lowest entry of the batch.
// PTLS_MI355X_COMBINE=k turns it on with k launches in flight per kind (default 0: every call on its own). Measured
// (tools/mt_records.c, 1200-byte seals): while a call waited for its stream's completion signal, 16 threads made 222K
// calls/s on their own and 264-269K combined (2.7 calls a launch). Once calls poll their completion words (roundtrip)
// a lone call is cheaper than a share of a batch: 16 threads 302K calls/s on their own against 249K combined (16 B:
// 352K / 270K; 16 KiB: 179K / 189K), so combining is off by default
// (profiles/r2_per_record/final_mt_and_skew.txt).

struct OneCall {
    ptls_mi355x_keyset_t *ks;
    size_t key_idx;
    bool open;
    void *output;
    const ptls_mi355x_iovec_t *vec;
    size_t incnt, len;
    uint64_t seq;
    const void *aad;
    size_t aadlen;
    int *verified;
    ptls_mi355x_keyset_t *hp_ks;  // header-protection mask of the sealed output's sample (fusion's supp) when set
    size_t hp_key_idx, sample_off;
    void *mask;
    int ret = -1;
    char err[sizeof(g_err)] = {};
    std::atomic<bool> done{false};
    const KeyEntry *entry() const { return ks->d_keys + key_idx; }
    const KeyEntry *hp_entry() const { return hp_ks->d_keys + hp_key_idx; }
};

#define COMBINE_MAX_CALLS 256               // calls per combined launch
#define COMBINE_MAX_BYTES ((size_t)65536)   // larger records and AADs run on their own
#ifndef COMBINE_WAIT_US
#define COMBINE_WAIT_US 5                   // how long a call that could lead waits for the rest of the last batch's callers
#endif


// Runs the calls `c[0..n)` (all of one kind) as one batch through one staging buffer and sets each call's ret (and
// err), then its done flag. Staging layout: [descriptors | hp entries | every call's input and AAD] is read by the
// device, [every call's output | ok bytes | masks] written (the copy path moves the first part up, the second down).
static void run_calls(DeviceState *ds, OneCall *const *c, size_t n)
{
    const auto t_start = std::chrono::steady_clock::now();
    const OneCall &c0 = *c[0];
    const bool open = c0.open, hp = c0.hp_ks != nullptr;
    const int nr = c0.ks->nr, hp_nr = hp ? c0.hp_ks->nr : 0;
    auto a16 = [](size_t x) { return (x + 15) & ~(size_t)15; };
    // the key indices of the batch: entries from the lowest one of the batch (all of them one-key slab entries when
    // n > 1; a lone call uses its own keyset's entries as they are)
    const KeyEntry *kbase = c0.entry(), *hbase = hp ? c0.hp_entry() : nullptr;
    for (size_t i = 1; i < n; ++i) {
        kbase = c[i]->entry() < kbase ? c[i]->entry() : kbase;
        if (hp)
            hbase = c[i]->hp_entry() < hbase ? c[i]->hp_entry() : hbase;
    }
    const size_t off_rec = 0, off_hp = a16(n * sizeof(ptls_mi355x_record_t)), off_data = off_hp + a16(n * sizeof(ptls_mi355x_hp_t));
    size_t up = off_data;
    for (size_t i = 0; i < n; ++i)
        up += a16(c[i]->len + (open ? 16 : 0)) + a16(c[i]->aadlen);
    size_t off_ok = up;
    for (size_t i = 0; i < n; ++i)
        off_ok += a16(c[i]->len + (open ? 0 : 16));
    // a lone long record runs over many workgroups (launch_span): 16-step units in spans of 2^e, at most one span per CU
    u32 span_units = 0, span_e = 0, span_n = 0;
    if (SPAN_MIN_BYTES != 0 && n == 1 && c0.len >= SPAN_MIN_BYTES && c0.ks->schedule != PTLS_MI355X_SCHEDULE_LOCKSTEP) {
        const size_t steps = ((c0.aadlen + 15) / 16 + (c0.len + 15) / 16 + 1 + ENGINE_G - 1) / ENGINE_G;
        span_units = (u32)((steps + CHUNK_STEPS - 1) / CHUNK_STEPS);
        const u32 cap = ds->ncu < 256 ? (u32)ds->ncu : 256u;
        while (((span_units + (1u << span_e) - 1) >> span_e) > cap)
            ++span_e;
        span_n = (span_units + (1u << span_e) - 1) >> span_e;
        if ((1u << span_e) > SPAN_MAX_UNITS)
            span_units = span_e = span_n = 0;
    }
    // header-protection masks: computed by the chunked seal launch itself (BatchArgs::hp), else by a second launch
    // (hp_kernel) after the lockstep seal, or after the span kernels
    const bool hp_fused = hp && span_n == 0 && runs_chunked(c0.ks);
    // completion words: one per workgroup of the last kernel (the GCM launch: one workgroup per record up to the CU
    // count; the header-protection launch: aux_grid)
    const size_t nflags = hp && !hp_fused ? (size_t)aux_grid(n, ds->ncu) : (n < (size_t)ds->ncu ? n : (size_t)ds->ncu);
    const size_t off_mask = off_ok + a16(n), off_flag = off_mask + 16 * n, off_span = off_flag + a16(4 * nflags),
                 total = off_span + 16 * (size_t)span_n;
    int ret = -1;
    {
        StageCall call(ds);
        // the plaintext side: a seal's inputs (up), an open's outputs (down); the copy path's device buffer is not cleared
        if (open)
            call.clear_lo = up;
        else
            call.clear_hi = up;
        if (call.acquire(total) == 0) {
            uint8_t *h = call.host(), *d = call.dev();
            const hipStream_t s = call.stream();
            u32 nkeys = 1, hp_nkeys = 1;
            size_t in_at = off_data, out_at = up;
            ptls_mi355x_record_t first = {};
            ret = 0;
            for (size_t i = 0; i < n && ret == 0; ++i) {
                const OneCall &x = *c[i];
                const size_t kd = (size_t)(x.entry() - kbase);
                const size_t inbytes = x.len + (open ? 16 : 0);
                gather_iovec(h + in_at, x.vec, x.incnt);
                const size_t aad_at = in_at + a16(inbytes);
                if (x.aadlen != 0)
                    memcpy(h + aad_at, x.aad, x.aadlen);
                const ptls_mi355x_record_t r = {in_at, out_at, x.seq, (u32)aad_at, (u32)x.len, (u32)kd, (uint16_t)x.aadlen,
                                                (uint16_t)(x.aadlen >> 16)};
                memcpy(h + off_rec + i * sizeof(r), &r, sizeof(r));
                if (i == 0)
                    first = r;
                nkeys = (u32)kd + 1 > nkeys ? (u32)kd + 1 : nkeys;
                if (hp) {
                    const size_t hd = (size_t)(x.hp_entry() - hbase);
                    const ptls_mi355x_hp_t e = {out_at + x.sample_off, (u32)hd, 0};
                    memcpy(h + off_hp + i * sizeof(e), &e, sizeof(e));
                    hp_nkeys = (u32)hd + 1 > hp_nkeys ? (u32)hd + 1 : hp_nkeys;
                }
                in_at = aad_at + a16(x.aadlen);
                out_at += a16(x.len + (open ? 0 : 16));
                if (wait_ready(x.ks, s) != 0 || (hp && wait_ready(x.hp_ks, s) != 0))
                    ret = -1;
            }
            // one record on one workgroup: shorter units put more of its waves to work (a unit step costs a lone
            // wave ~2 us of latency, a unit combine ~0.15 us); steps / 2^k units balance the two (tools/latency.py).
            // Long records, and batches (one workgroup per record), pass CHUNK_LOG2: the kernel's scan then picks.
            const size_t steps = ((c0.aadlen + 15) / 16 + (c0.len + 15) / 16 + 1 + ENGINE_G - 1) / ENGINE_G;
            const u32 unit_log2 = n > 1 ? CHUNK_LOG2 : steps <= 24 ? 0 : steps <= 96 ? 1 : steps <= 400 ? 2 : steps <= 1600 ? 3 : CHUNK_LOG2;
            // (calls staging at most 1 MiB: a larger record's launch runs for hundreds of microseconds or more, which
            // the caller need not spend spinning on a core)
            const bool flag = call.mapped() && c0.ks->schedule != PTLS_MI355X_SCHEDULE_LOCKSTEP &&
                              (total <= PERREC_FLAG_MAX_BYTES || span_n != 0);
            // this call's completion token (never 0, and never the value an earlier call left in these words)
            const u32 token = flag ? next_done_token() : 0u;
            if (flag)
                memset(h + off_flag, 0, 4 * nflags);
            if (ret == 0)
                ret = call.roundtrip(up, [&] {
                    // (the completion words belong to the call's last kernel: the header-protection launch if not fused)
                    const HpLaunch hpl = {(const ptls_mi355x_hp_t *)(d + off_hp), hbase, hp_nkeys, hp_nr, d + off_mask};
                    GcmLaunch g = {};
                    g.a.keys = kbase, g.a.nkeys = nkeys, g.a.recs = (const ptls_mi355x_record_t *)(d + off_rec), g.a.nrecs = n;
                    g.a.in = g.a.aad = g.a.out = d, g.a.ok = d + off_ok, g.a.unit_log2 = unit_log2;
                    g.a.done_flag = flag && (!hp || hp_fused) ? (u32 *)(d + off_flag) : nullptr, g.a.done_token = token;
                    g.stream = s, g.nr = nr, g.ncu = ds->ncu, g.schedule = c0.ks->schedule, g.ct = c0.ks->ct, g.open = open;
                    g.hp = hp_fused ? &hpl : nullptr;  // (never with a span)
                    g.one = n == 1 ? &first : nullptr;
                    if ((span_n != 0 ? launch_span(g, span_units, span_e, span_n, d + off_span) : launch_gcm(g)) != 0)
                        return -1;
                    return !hp || hp_fused ? 0
                               : launch_hp(hbase, hp_nkeys, hp_nr, ds->ncu, (const ptls_mi355x_hp_t *)(d + off_hp), n, d, d + off_mask, s,
                                           flag ? (u32 *)(d + off_flag) : nullptr, token);
                }, flag ? off_flag : 0, nflags, token);
            if (ret == 0) {
                out_at = up;
                for (size_t i = 0; i < n; ++i) {
                    OneCall &x = *c[i];
                    seen_ready(x.ks);
                    if (hp)
                        seen_ready(x.hp_ks);
                    const size_t outbytes = x.len + (open ? 0 : 16);
                    if (outbytes != 0)
                        memcpy(x.output, h + out_at, outbytes);
                    if (open)
                        *x.verified = h[off_ok + i];
                    if (hp)
                        memcpy(x.mask, h + off_mask + 16 * i, 16);
                    out_at += a16(outbytes);
                }
                if (ds->diag && flag && call.mapped()) {
                    // (diagnosis: did any result byte change after the completion words were seen?)
                    (void)hipStreamSynchronize(s);
                    size_t at = up;
                    for (size_t i = 0; i < n; ++i) {
                        const OneCall &x = *c[i];
                        const size_t outbytes = x.len + (open ? 0 : 16);
                        size_t diff = 0, first = SIZE_MAX;
                        for (size_t b = 0; b < outbytes; ++b)
                            if (h[at + b] != ((const uint8_t *)x.output)[b])
                                diff++, first = first == SIZE_MAX ? b : first;
                        const bool okchg = open && h[off_ok + i] != (uint8_t)*x.verified;
                        if (diff != 0 || okchg)
                            fprintf(stderr, "ptls_mi355x diag: %s of %zu bytes: %zu result bytes (first at %zu)%s changed after the "
                                            "completion words were seen\n", open ? "open" : "seal", x.len, diff,
                                    first == SIZE_MAX ? (size_t)0 : first, okchg ? " and the ok byte" : "");
                        at += a16(outbytes);
                    }
                }
            }
        }
    }
    if (g_cstats.on) {
        g_cstats.launches += 1, g_cstats.calls += n;
        g_cstats.ns += (uint64_t)std::chrono::duration_cast<std::chrono::nanoseconds>(std::chrono::steady_clock::now() - t_start).count();
    }
    for (size_t i = 0; i < n; ++i) {
        c[i]->ret = ret;
        if (ret != 0)
            memcpy(c[i]->err, g_err, sizeof(g_err));
        c[i]->done.store(true, std::memory_order_release);
    }
}

// the combiner of a call's kind (index into DeviceState::comb), or -1 when the call runs on its own
static int combine_kind(const OneCall &c)
{
    if (!c.ks->slot || c.ks->schedule == PTLS_MI355X_SCHEDULE_LOCKSTEP || c.len > COMBINE_MAX_BYTES || c.aadlen > COMBINE_MAX_BYTES ||
        (c.hp_ks != nullptr && !c.hp_ks->slot))
        return -1;
    return (c.open ? 1 : 0) | (c.ks->nr == 14 ? 2 : 0) | (c.ks->ct ? 4 : 0) | (c.hp_ks == nullptr ? 0 : c.hp_ks->nr == 14 ? 16 : 8);
}

static int submit(DeviceState *ds, OneCall *c)
{
    const int kind = ds->combine > 0 ? combine_kind(*c) : -1;
    if (kind < 0) {
        run_calls(ds, &c, 1);
    } else {
        Combiner &cb = ds->comb[kind];
        std::vector<OneCall *> batch;
        const auto t_enq = std::chrono::steady_clock::now();
        std::unique_lock<std::mutex> lk(cb.mu);
        cb.q.push_back(c);
        while (!c->done.load(std::memory_order_acquire)) {
            // a launch slot is free: take the queue -- unless fewer calls have queued than the last batch held and this
            // call has waited less than COMBINE_WAIT_US: threads whose calls just completed are about to submit their
            // next ones, and a batch taken at once would hold only the first of them (a lone caller never waits)
            if (cb.inflight < ds->combine && !cb.q.empty() &&
                (cb.q.size() >= cb.expect ||
                 std::chrono::steady_clock::now() - t_enq >= std::chrono::microseconds(COMBINE_WAIT_US))) {
                // as many queued calls as fit one staging buffer (each call's share is about its bytes up and down)
                size_t take = 0, bytes = 0;
                while (take < cb.q.size() && take < COMBINE_MAX_CALLS) {
                    const OneCall &x = *cb.q[take];
                    bytes += 2 * x.len + x.aadlen + 128;
                    if (take > 0 && bytes > ds->stage_limit / 2)
                        break;
                    ++take;
                }
                batch.assign(cb.q.begin(), cb.q.begin() + (long)take);
                cb.q.erase(cb.q.begin(), cb.q.begin() + (long)take);
                ++cb.inflight;
                cb.expect = take;
                lk.unlock();
                // a batch's calls address their entries as key indices from its lowest entry, which is defined only
                // within one slab (slabs are separate allocations): calls whose entries lie in several slabs run one
                // by one
                auto one_slab = [&](bool hp_entries) {
                    const KeyEntry *slab = hp_entries ? batch[0]->hp_ks->slab : batch[0]->ks->slab;
                    for (OneCall *x : batch)
                        if ((hp_entries ? x->hp_ks->slab : x->ks->slab) != slab)
                            return false;
                    return true;
                };
                if (batch.size() == 1 || (one_slab(false) && (batch[0]->hp_ks == nullptr || one_slab(true)))) {
                    run_calls(ds, batch.data(), batch.size());
                } else {
                    for (OneCall *x : batch)
                        run_calls(ds, &x, 1);
                }
                lk.lock();
                --cb.inflight;
                continue;
            }
            lk.unlock();
            for (int k = 0; k < 256 && !c->done.load(std::memory_order_acquire); ++k)
                __builtin_ia32_pause();
            if (!c->done.load(std::memory_order_acquire))
                sched_yield();
            lk.lock();
        }
    }
    if (c->ret != 0)
        return fail("%s", c->err);
    return 0;
}

// one record on host buffers (input as iovecs), optionally with the header-protection mask of a sample of the sealed
// output under hp_ks (fusion's supp, lib/fusion.c:425-430,636-651): a batch of one through a staging buffer, or a
// share of a batch combined with other threads' calls (submit)
static int single(ptls_mi355x_keyset_t *ks, size_t key_idx, bool open, void *output, const ptls_mi355x_iovec_t *vec, size_t incnt,
                  size_t len, uint64_t seq, const void *aad, size_t aadlen, int *verified, ptls_mi355x_keyset_t *hp_ks = NULL,
                  size_t hp_key_idx = 0, size_t sample_off = 0, void *mask = NULL)
{
    if (check_single_args("single", ks != NULL && key_idx < ks->nkeys, aad, aadlen, output, len) != 0)
        return -1;
    if (hp_ks != NULL && (hp_key_idx >= hp_ks->nkeys || hp_ks->device != ks->device || sample_off > len))
        return fail("%s", "single: invalid header-protection arguments");
    DeviceScope scope(ks->device);
    OneCall c;
    c.ks = ks, c.key_idx = key_idx, c.open = open, c.output = output, c.vec = vec, c.incnt = incnt, c.len = len, c.seq = seq;
    c.aad = aad, c.aadlen = aadlen, c.verified = verified, c.hp_ks = hp_ks, c.hp_key_idx = hp_key_idx;
    c.sample_off = sample_off, c.mask = mask;
    return submit(ks->ds, &c);
}

extern "C" {

int ptls_mi355x_encrypt(ptls_mi355x_keyset_t *ks, size_t key_idx, void *output, const void *input, size_t inlen, uint64_t seq,
                        const void *aad, size_t aadlen)
{
    const ptls_mi355x_iovec_t v = {input, inlen};
    return single(ks, key_idx, false, output, &v, 1, inlen, seq, aad, aadlen, NULL);
}

int ptls_mi355x_encrypt_v(ptls_mi355x_keyset_t *ks, size_t key_idx, void *output, const ptls_mi355x_iovec_t *input, size_t incnt,
                          uint64_t seq, const void *aad, size_t aadlen)
{
    size_t len = 0;
    for (size_t i = 0; i < incnt; ++i) {
        if (input[i].len != 0 && input[i].base == NULL)
            return fail("%s", "encrypt_v: invalid iovec");
        len += input[i].len;
    }
    return single(ks, key_idx, false, output, input, incnt, len, seq, aad, aadlen, NULL);
}

int ptls_mi355x_encrypt_s(ptls_mi355x_keyset_t *ks, size_t key_idx, void *output, const void *input, size_t inlen, uint64_t seq,
                          const void *aad, size_t aadlen, ptls_mi355x_keyset_t *hp_ks, size_t hp_key_idx, size_t sample_off,
                          void *mask)
{
    if (hp_ks == NULL || mask == NULL)
        return fail("%s", "encrypt_s: invalid arguments");
    const ptls_mi355x_iovec_t v = {input, inlen};
    return single(ks, key_idx, false, output, &v, 1, inlen, seq, aad, aadlen, NULL, hp_ks, hp_key_idx, sample_off, mask);
}

size_t ptls_mi355x_decrypt(ptls_mi355x_keyset_t *ks, size_t key_idx, void *output, const void *input, size_t inlen, uint64_t seq,
                           const void *aad, size_t aadlen)
{
    if (inlen < 16)
        return SIZE_MAX;
    int verified = 0;
    const ptls_mi355x_iovec_t v = {input, inlen};
    if (single(ks, key_idx, true, output, &v, 1, inlen - 16, seq, aad, aadlen, &verified) != 0)
        return SIZE_MAX;
    return verified ? inlen - 16 : SIZE_MAX;
}

int ptls_mi355x_quiclb_transform(ptls_mi355x_keyset_t *ks, size_t key_idx, void *output, const void *input, size_t len, int encrypt)
{
    if (ks == NULL || key_idx >= ks->nkeys || output == NULL || input == NULL || len < PTLS_MI355X_QUICLB_MIN_LEN ||
        len > PTLS_MI355X_QUICLB_MAX_LEN || ks->key_size != 16)
        return fail("%s", "quiclb_transform: invalid arguments");
    DeviceScope scope(ks->device);
    StageCall call(ks->ds);
    // staging: [0, 32) CID in, [32, 56) descriptor | [64, 96) CID out
    if (call.acquire(96) != 0)
        return -1;
    const ptls_mi355x_cid_t c = {0, 64, 0, (uint8_t)len, (uint8_t)(encrypt != 0), 0};
    memcpy(call.host(), input, len);
    memcpy(call.host() + 32, &c, sizeof(c));
    uint8_t *d = call.dev();
    const hipStream_t s = call.stream();
    if (wait_ready(ks, s) != 0 || call.roundtrip(64, [&] {
            quiclb_kernel<10><<<1, 256, LDS_AES_BYTES, s>>>(ks->d_keys + key_idx, 1, (const ptls_mi355x_cid_t *)(d + 32), d, d, 1);
            HIP_TRY(hipGetLastError());
            return 0;
        }) != 0)
        return -1;
    seen_ready(ks);
    memcpy(output, call.host() + 64, len);
    return 0;
}

int ptls_mi355x_encrypt_blocks(ptls_mi355x_keyset_t *ks, size_t key_idx, void *out, const void *in, size_t nblocks)
{
    if (ks == NULL || key_idx >= ks->nkeys || (nblocks != 0 && (out == NULL || in == NULL)) || nblocks > ((size_t)1 << 26))
        return fail("%s", "encrypt_blocks: invalid arguments");
    if (nblocks == 0)
        return 0;
    DeviceScope scope(ks->device);
    StageCall call(ks->ds);
    // staging: [0, n) blocks in | [n', n' + n) blocks out, n' = n rounded up to 32 bytes
    const size_t n = nblocks * 16, up = (n + 31) & ~(size_t)31;
    if (call.acquire(2 * up) != 0)
        return -1;
    memcpy(call.host(), in, n);
    uint8_t *d = call.dev();
    const hipStream_t s = call.stream();
    if (wait_ready(ks, s) != 0 ||
        call.roundtrip(up, [&] { return launch_ecb(ks->d_keys + key_idx, 1, ks->nr, ks->ds->ncu, NULL, d, d + up, nblocks, s); }) != 0)
        return -1;
    seen_ready(ks);
    memcpy(out, call.host() + up, n);
    return 0;
}

int ptls_mi355x_encrypt_block(ptls_mi355x_keyset_t *ks, size_t key_idx, void *out, const void *in)
{
    if (ks == NULL || key_idx >= ks->nkeys || out == NULL || in == NULL)
        return fail("%s", "encrypt_block: invalid arguments");
    return ptls_mi355x_encrypt_blocks(ks, key_idx, out, in, 1);
}

}  // extern "C"

#endif  // PTLS_MI355X_HOST_AESGCM_H
