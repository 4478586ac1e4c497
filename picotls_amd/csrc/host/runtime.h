// picotls_amd/csrc/host/runtime.h -- the host runtime both AEAD families share: error reporting, the per-device state
// and its pools (events, one-key slab entries, staging buffers), the synchronous staging round trip, the record of a
// keyset's launches (StreamUses), its scratch blocks (Scratch), per-stream slots (StreamSlots), the run-time -> template dispatch helpers and what a
// call on two keysets needs (QUIC packets: argument check, PairLock, launch_and_note_both).
// Part of the single translation unit picotls_amd/csrc/aesgcm_engine.hip (included after the device code; not standalone).
#ifndef PTLS_MI355X_HOST_RUNTIME_H
#define PTLS_MI355X_HOST_RUNTIME_H

static thread_local char g_err[256];

static int fail(const char *fmt, const char *detail)
{
    snprintf(g_err, sizeof(g_err), fmt, detail);
    return -1;
}

// Kernel launches are checked with hipGetLastError, which also returns the error of any earlier call of this thread
// whose failure was handled (a failed hipHostGetDevicePointer, for one: tools/mb/lasterr.hip showed that error reported
// after a good launch). LAUNCH_CLEAR() before a launch makes the check after it about that launch only.
// (-DLAUNCH_CLEAR_NOOP=1: a tools/ variant without it, which the regression test of tests/c/test_vtable.c `lasterr`
// must fail on; never the shipped build)
#if LAUNCH_CLEAR_NOOP
#define LAUNCH_CLEAR() ((void)0)
#else
#define LAUNCH_CLEAR() ((void)hipGetLastError())
#endif

#define HIP_TRY(expr)                                                                                                         \
    do {                                                                                                                      \
        hipError_t e_ = (expr);                                                                                               \
        if (e_ != hipSuccess)                                                                                                 \
            return fail(#expr ": %s", hipGetErrorString(e_));                                                                 \
    } while (0)

static void clear_memory(void *p, size_t n)  // ptls_clear_memory: a memset the compiler may not drop
{
    volatile uint8_t *v = (volatile uint8_t *)p;
    while (n-- != 0)
        *v++ = 0;
}

// ---- per-device state
//
// picotls contexts are independent (lib/picotls.c:6553-6568: a context is malloc'd, set up and freed by its owner,
// fusion's setup touches nothing shared; SURVEY 8(b) Threading), and a QUIC or TLS server creates and frees them per
// connection and epoch. So nothing here waits for the whole device (no hipDeviceSynchronize, no hipFree, whose implicit
// device-wide synchronisation would stall every batch in flight):
//   * one-key keysets (a picotls context) take a 512-byte entry from a per-device slab and are set up by one launch whose
//     key travels in the kernel arguments, on the device's setup stream, with an event their first use waits for;
//   * teardown, rekey and IV changes run on the device's maintenance stream, ordered after the keyset's own launches
//     (an event per stream it was used on), and a freed slab entry returns to the pool only once it has been cleared;
//   * the synchronous host-buffer helpers (the per-record picotls path) take a staging buffer and its stream from a
//     per-device pool for the duration of one call, so concurrent contexts on different threads never share one.

#define MAX_DEVICES 64
#define STAGE_CLASSES 26   // pinned staging buffers of 4 KiB << class
#define SLAB_ENTRIES 1024  // one-key keyset entries per slab (512 KiB)
// Bounds of the staging pool (fusion's context owns one allocation and frees it, lib/fusion.c:1043-1049; here the pinned
// buffers outlive calls so that the next call of a thread skips hipHostMalloc, but not without limit):
#define STAGE_POOL_BYTES ((size_t)64 << 20)  // idle pinned bytes kept per device (PTLS_MI355X_STAGE_POOL_BYTES)
#define STAGE_KEEP_MAX ((size_t)16 << 20)     // a buffer above this (a call of a record > ~8 MiB) is freed after its call
#define STAGE_STREAMS 16                      // stager streams per device, shared round-robin beyond that

struct Stager {
    hipStream_t stream;  // one of the device's stager streams (DeviceState::stage_streams), not owned
    uint8_t *h;      // pinned host buffer
    uint8_t *h_dev;  // its device address (NULL: not mapped, or PTLS_MI355X_STAGE_COPY=1: round trips copy through d)
    uint8_t *d;      // device buffer of the copy path
    size_t cap;
    int cls;
    Stager *next;
};

struct PendingSlot {
    KeyEntry *e;
    KeyEntry *slab;
    hipEvent_t cleared;
};

struct OneCall;
struct Combiner {  // per-record calls of one kind waiting for a launch (submit)
    std::mutex mu;
    std::vector<OneCall *> q;
    int inflight = 0;
    size_t expect = 1;  // calls in the last batch: a caller that could lead waits briefly until as many have queued
};

struct DeviceState {
    int device = 0, ncu = 0;
    hipStream_t setup = nullptr;  // one-key and many-key setup launches (never waits on anything)
    hipStream_t maint = nullptr;  // teardown, rekey, set_iv: ordered after the keyset's launches
    int priority = 0;             // the device's greatest stream priority: the engine's own streams (setup, teardown,
                                  // per-record round trips) are dispatched ahead of bulk batches on ordinary streams
    bool force_copy = false;      // PTLS_MI355X_STAGE_COPY=1: the staging round trip copies instead of mapping
    bool stage_coherent = true;   // staging buffers fine-grained (hipHostMallocCoherent); PTLS_MI355X_STAGE_COHERENT=0: the
                                  // HIP default (coarse-grained), kept only to reproduce the round-3 race
    size_t stage_limit = 0;       // PTLS_MI355X_MAX_STAGE_BYTES: the largest staging buffer one call may use
    bool ct_default = true;       // new keysets are constant-time (PTLS_MI355X_CONSTANT_TIME=0: not, for an A/B)
    bool fault_order = false;     // PTLS_MI355X_FAULT_ORDER=1 (tests only): keyset teardown cannot order itself on the device
    bool diag = false;            // PTLS_MI355X_DIAG=1 (diagnosis only): per-record calls re-read their results after a stream
                                  // synchronisation and report bytes that changed after the completion words were seen
    std::mutex mu;                // the pools below
    Stager *stagers[STAGE_CLASSES] = {};
    size_t stage_idle = 0;        // pinned bytes of the idle stagers above
    size_t stage_busy = 0;        // ... and of the stagers in use by calls
    size_t stage_pool_cap = STAGE_POOL_BYTES;
    std::vector<hipStream_t> stage_streams;  // at most STAGE_STREAMS
    unsigned stage_rr = 0;
    std::vector<std::pair<KeyEntry *, KeyEntry *>> slots;  // free one-key entries and the slab each lies in
    std::vector<PendingSlot> pending;
    std::vector<std::pair<void *, hipEvent_t>> frees;  // retired blocks until the event behind their last user has completed (retire_after)
    std::vector<hipEvent_t> events;
    int combine = 0;              // PTLS_MI355X_COMBINE: combined per-record launches in flight per kind (0: none)
    Combiner comb[32];
};

static std::atomic<DeviceState *> g_devs[MAX_DEVICES];
static std::mutex g_devs_mu;

static int set_kernel_attrs(void);  // (host/aesgcm.h: the AES-GCM kernels' dynamic LDS sizes)

// The state of HIP device `dev` (the current device of the calling thread), created on first use under a lock; it
// lives as long as the process (it holds the pools).
static DeviceState *device_state(int dev)
{
    if (dev < 0 || dev >= MAX_DEVICES) {
        fail("%s", "device index out of range");
        return nullptr;
    }
    DeviceState *ds = g_devs[dev].load(std::memory_order_acquire);
    if (ds != nullptr)
        return ds;
    std::lock_guard<std::mutex> lk(g_devs_mu);
    if ((ds = g_devs[dev].load(std::memory_order_relaxed)) != nullptr)
        return ds;
    ds = new (std::nothrow) DeviceState();
    if (ds == nullptr) {
        fail("%s", "out of memory");
        return nullptr;
    }
    ds->device = dev;
    const char *copy = getenv("PTLS_MI355X_STAGE_COPY"), *limit = getenv("PTLS_MI355X_MAX_STAGE_BYTES");
    ds->force_copy = copy != nullptr && strcmp(copy, "1") == 0;
    const char *coh = getenv("PTLS_MI355X_STAGE_COHERENT");
    ds->stage_coherent = !(coh != nullptr && strcmp(coh, "0") == 0);
    const char *ct = getenv("PTLS_MI355X_CONSTANT_TIME");
    // (round 4) every keyset constant-time unless PTLS_MI355X_CONSTANT_TIME=0: since the window-major segment ends
    // both modes run the same code, whose LDS accesses have data-independent bank patterns, at the same
    // rate; the flag only keeps such keysets off the lockstep schedule
    ds->ct_default = !(ct != nullptr && strcmp(ct, "0") == 0);
    const char *comb = getenv("PTLS_MI355X_COMBINE");
    if (comb != nullptr)
        ds->combine = atoi(comb) < 0 ? 0 : atoi(comb);
    const char *pool = getenv("PTLS_MI355X_STAGE_POOL_BYTES"), *fo = getenv("PTLS_MI355X_FAULT_ORDER");
    if (pool != nullptr)
        ds->stage_pool_cap = (size_t)strtoull(pool, nullptr, 0);
    ds->fault_order = fo != nullptr && strcmp(fo, "1") == 0;
    const char *dg = getenv("PTLS_MI355X_DIAG");
    ds->diag = dg != nullptr && strcmp(dg, "1") == 0;
    ds->stage_limit = limit != nullptr ? (size_t)strtoull(limit, nullptr, 0) : (size_t)4096 << (STAGE_CLASSES - 1);
    int least = 0;
    if (hipDeviceGetStreamPriorityRange(&least, &ds->priority) != hipSuccess)
        ds->priority = 0;
    if (hipDeviceGetAttribute(&ds->ncu, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || set_kernel_attrs() != 0 ||
        hipStreamCreateWithPriority(&ds->setup, hipStreamNonBlocking, ds->priority) != hipSuccess ||
        hipStreamCreateWithPriority(&ds->maint, hipStreamNonBlocking, ds->priority) != hipSuccess) {
        if (ds->setup != nullptr)
            (void)hipStreamDestroy(ds->setup);
        delete ds;
        fail("%s", "device initialisation failed");
        return nullptr;
    }
    g_devs[dev].store(ds, std::memory_order_release);
    return ds;
}

static DeviceState *current_device_state(void)
{
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess) {
        fail("%s", "hipGetDevice failed");
        return nullptr;
    }
    return device_state(dev);
}

// makes `dev` the calling thread's current device for the scope of a call (a context may be used from a thread whose
// current device is another one), restoring the previous one after
struct DeviceScope {
    int prev = -1;
    explicit DeviceScope(int dev)
    {
        int cur = 0;
        if (hipGetDevice(&cur) == hipSuccess && cur != dev && hipSetDevice(dev) == hipSuccess)
            prev = cur;
    }
    ~DeviceScope()
    {
        if (prev >= 0)
            (void)hipSetDevice(prev);
    }
};

static hipEvent_t event_get(DeviceState *ds)
{
    {
        std::lock_guard<std::mutex> lk(ds->mu);
        if (!ds->events.empty()) {
            hipEvent_t e = ds->events.back();
            ds->events.pop_back();
            return e;
        }
    }
    hipEvent_t e = nullptr;
    if (hipEventCreateWithFlags(&e, hipEventDisableTiming) != hipSuccess)
        return nullptr;
    return e;
}

static void event_put(DeviceState *ds, hipEvent_t e)
{
    if (e == nullptr)
        return;
    std::lock_guard<std::mutex> lk(ds->mu);
    ds->events.push_back(e);
}

// Retires a block of stream-ordered memory whose last possible user is queued on `behind` (or ordered before what is):
// an event is recorded there, and the block goes back to the pool (hipFreeAsync) only once that event has completed,
// checked by the keyset calls that follow (`p` null: only that check). Nothing waits on the host. hipFreeAsync at
// once is not enough, on whichever stream: the pool takes the stream a block was allocated on as safe for reuse
// without waiting, so the next keyset was handed a block freed on the maintenance stream and copied its keys into it
// while the freed keyset's last launch, on a third stream, was still reading it (tests/test_gpu_chacha.py, free and
// rekey right after a launch).
static void retire_after(DeviceState *ds, hipStream_t behind, void *p)
{
    std::vector<void *> idle;
    hipEvent_t done = p != nullptr ? event_get(ds) : nullptr;
    if (done != nullptr && hipEventRecord(done, behind) != hipSuccess) {
        event_put(ds, done);  // (the block is kept, never reused, rather than freed under a launch)
        done = nullptr;
    }
    {
        std::lock_guard<std::mutex> lk(ds->mu);
        if (done != nullptr)
            ds->frees.emplace_back(p, done);
        for (size_t i = 0; i < ds->frees.size();) {
            if (hipEventQuery(ds->frees[i].second) == hipSuccess) {
                idle.push_back(ds->frees[i].first);
                ds->events.push_back(ds->frees[i].second);
                ds->frees[i] = ds->frees.back();
                ds->frees.pop_back();
            } else {
                (void)hipGetLastError();  // (not ready: not an error for the launches that follow)
                ++i;
            }
        }
    }
    for (void *q : idle)
        (void)hipFreeAsync(q, ds->maint);
}

// ... a freed keyset's entries, their clearing just queued on the maintenance stream
static void free_after_maint(DeviceState *ds, void *entries) { retire_after(ds, ds->maint, entries); }

// Which launches used a keyset: per stream it was used on, an event recorded after its last launch there. Teardown,
// rekey and IV changes order themselves after all of them; a stream that takes over another stream's scratch or slot
// waits for that stream's. The keyset's mutex guards it.
struct StreamUses {
    std::vector<std::pair<hipStream_t, hipEvent_t>> uses;
    hipEvent_t event_of(hipStream_t s) const  // the use event of `s` (null: the keyset was never used on it)
    {
        const auto it = std::find_if(uses.begin(), uses.end(), [s](auto &u) { return u.first == s; });
        return it != uses.end() ? it->second : nullptr;
    }
    // records that the keyset was used by work just launched on `s`
    int note(DeviceState *ds, hipStream_t s)
    {
        hipEvent_t e = event_of(s);
        if (e == nullptr) {
            if ((e = event_get(ds)) == nullptr)
                return fail("%s", "event creation failed");
            uses.emplace_back(s, e);
        }
        return hipEventRecord(e, s) == hipSuccess ? 0 : fail("%s", "hipEventRecord failed");
    }
    int order_after_all(hipStream_t stream) const  // `stream` waits for every recorded use
    {
        for (auto &u : uses)
            HIP_TRY(hipStreamWaitEvent(stream, u.second, 0));
        return 0;
    }
    bool drain() const  // the host waits for every recorded use; false when one of the waits failed
    {
        return std::count_if(uses.begin(), uses.end(), [](auto &u) { return hipEventSynchronize(u.second) != hipSuccess; }) == 0;
    }
    void release(DeviceState *ds)
    {
        for (auto &u : uses)
            event_put(ds, u.second);
        uses.clear();
    }
};

// `launch()`, then the keyset's use on `s` -- recorded whether or not the launch failed: a failed launch may have queued
// part of its work (EXT 4 of a W8 pair before its EXT 3 failed, for one), and teardown, a takeover of the stream's slot and a
// scratch regrow wait for whatever was queued. The launch's error is the one reported; `uses` is locked.
template <typename Launch>
static int launch_and_note(StreamUses &uses, DeviceState *ds, hipStream_t s, Launch launch)
{
    if (launch() == 0)
        return uses.note(ds, s);
    char err[sizeof(g_err)];
    memcpy(err, g_err, sizeof(err));
    (void)uses.note(ds, s);
    memcpy(g_err, err, sizeof(err));
    return -1;
}

// A block of device scratch that a keyset lends to its launches on any stream: allocated in stream order by the first
// launch that needs it, regrown when one needs more, retired with the keyset. Two rules keep it from being read and
// written, or handed out again, under a launch still using it:
//   * a launch on another stream than the last user's first waits for that stream's use event (StreamUses) -- so every
//     launch that takes the block must be noted (launch_and_note) before the keyset's mutex is released; back-to-back
//     launches on one stream add no event packets (a wait and a record per launch cost a 23 us small-batch launch 7 us);
//   * a block outgrown (behind `s`, which by then waits for the last user) or released (behind the maintenance stream,
//     ordered after every use) goes through retire_after, never to hipFreeAsync directly.
// The keyset's mutex guards it, held from take() through the launch and its use event.
struct Scratch {
    void *p = nullptr;
    size_t cap = 0;              // its bytes
    hipStream_t last = nullptr;  // the stream of its last user (while p is set)
    void retire(DeviceState *ds, hipStream_t behind)
    {
        if (p != nullptr)
            retire_after(ds, behind, p);
        p = nullptr, cap = 0;
    }
    // the block, of at least `bytes`, for a launch about to be made on `s`; a new block has its first `zero_prefix` bytes
    // zeroed. nullptr after a HIP failure (the error text set), the owner then empty: the caller decides whether its
    // launch can do without.
    void *take(DeviceState *ds, const StreamUses &uses, hipStream_t s, size_t bytes, size_t zero_prefix = 0)
    {
        const auto failed = [&](hipStream_t behind, const char *what, hipError_t e) {
            retire(ds, behind);
            (void)hipGetLastError();  // (handled: the launches that follow are checked with hipGetLastError)
            fail(what, hipGetErrorString(e));
            return nullptr;
        };
        hipError_t e;
        if (p != nullptr && last != s) {
            const hipEvent_t used = uses.event_of(last);
            if (used != nullptr && (e = hipStreamWaitEvent(s, used, 0)) != hipSuccess)
                return failed(last, "scratch: hipStreamWaitEvent: %s", e);
        }
        if (bytes > cap) {
            retire(ds, s);
            if ((e = hipMallocAsync(&p, bytes, s)) != hipSuccess) {
                p = nullptr;
                return failed(s, "scratch: hipMallocAsync: %s", e);
            }
            if (zero_prefix != 0 && (e = hipMemsetAsync(p, 0, zero_prefix, s)) != hipSuccess)
                return failed(s, "scratch: hipMemsetAsync: %s", e);
            cap = bytes;
        }
        last = s;
        return p;
    }
    // at teardown, the maintenance stream ordered after every use of the keyset (or the host having waited for them)
    void release(DeviceState *ds, bool clear)
    {
        if (clear && p != nullptr)
            (void)hipMemsetAsync(p, 0, cap, ds->maint);
        retire(ds, ds->maint);
    }
};

// At most CAP per-stream resources of a keyset (W8 flag buffers, ChaCha claim slots), most recently used last. A stream
// runs its launches in order, so a stream's own entry needs no further ordering; a new stream beyond CAP takes over
// the least recently used entry after waiting for the last use (StreamUses) of the stream that held it. The keyset's
// mutex guards it, held through the launch and its use event.
template <typename T, size_t CAP>
struct StreamSlots {
    std::vector<std::pair<hipStream_t, T>> v;
    // the entry of `s`, made by make(T &) (false: failed) for a new stream below CAP; nullptr on failure
    template <typename Make>
    T *get(hipStream_t s, const StreamUses &uses, Make make)
    {
        auto it = std::find_if(v.begin(), v.end(), [s](auto &e) { return e.first == s; });
        if (it == v.end() && v.size() < CAP) {
            T t{};
            if (!make(t))
                return nullptr;
            it = v.insert(it, {s, t});
        } else if (it == v.end()) {
            const hipEvent_t prev = uses.event_of(v.front().first);
            const hipError_t e = prev != nullptr ? hipStreamWaitEvent(s, prev, 0) : hipSuccess;
            if (e != hipSuccess) {
                fail("hipStreamWaitEvent: %s", hipGetErrorString(e));
                return nullptr;
            }
            (it = v.begin())->first = s;
        }
        std::rotate(it, it + 1, v.end());
        return &v.back().second;
    }
};

// one cleared keyset entry from the slab: a free one, else one whose clearing (keyset_free) has completed, else a new
// slab; *slab is the slab the entry lies in (entries of one slab may be addressed relative to each other)
static KeyEntry *slot_get(DeviceState *ds, KeyEntry **slab_of)
{
    {
        std::lock_guard<std::mutex> lk(ds->mu);
        if (ds->slots.empty()) {
            for (size_t i = 0; i < ds->pending.size();) {
                if (hipEventQuery(ds->pending[i].cleared) == hipSuccess) {
                    ds->slots.emplace_back(ds->pending[i].e, ds->pending[i].slab);
                    ds->events.push_back(ds->pending[i].cleared);
                    ds->pending[i] = ds->pending.back();
                    ds->pending.pop_back();
                } else {
                    (void)hipGetLastError();  // (not ready: not an error for the launches that follow)
                    ++i;
                }
            }
        }
        if (!ds->slots.empty()) {
            const auto e = ds->slots.back();
            ds->slots.pop_back();
            *slab_of = e.second;
            return e.first;
        }
    }
    KeyEntry *slab = nullptr;
    if (hipMalloc((void **)&slab, SLAB_ENTRIES * sizeof(KeyEntry)) != hipSuccess) {
        fail("%s", "keyset slab allocation failed");
        return nullptr;
    }
    std::lock_guard<std::mutex> lk(ds->mu);
    for (int i = SLAB_ENTRIES - 1; i >= 1; --i)
        ds->slots.emplace_back(slab + i, slab);
    *slab_of = slab;
    return slab;
}

static void stager_destroy(Stager *s)
{
    if (s->d != nullptr)
        (void)hipFree(s->d);
    (void)hipHostFree(s->h);  // (an implicit device synchronisation: only buffers beyond the pool's bounds get here)
    delete s;
}

// frees the idle staging buffers of one device (hipHostFree waits for that device)
static void release_idle_stagers(DeviceState *ds)
{
    std::vector<Stager *> idle;
    {
        std::lock_guard<std::mutex> lk(ds->mu);
        for (int c = 0; c < STAGE_CLASSES; ++c) {
            for (Stager *s = ds->stagers[c]; s != nullptr; s = s->next)
                idle.push_back(s);
            ds->stagers[c] = nullptr;
        }
        ds->stage_idle = 0;
    }
    for (Stager *s : idle)
        stager_destroy(s);
}

static Stager *stager_get(DeviceState *ds, size_t bytes)
{
    if (bytes > ds->stage_limit) {
        fail("%s", "staging: the call needs more than PTLS_MI355X_MAX_STAGE_BYTES");
        return nullptr;
    }
    int cls = 0;
    while (cls < STAGE_CLASSES && ((size_t)4096 << cls) < bytes)
        ++cls;
    if (cls == STAGE_CLASSES) {
        fail("%s", "staging: record too large");
        return nullptr;
    }
    hipStream_t stream = nullptr;
    {
        std::lock_guard<std::mutex> lk(ds->mu);
        Stager *s = ds->stagers[cls];
        if (s != nullptr) {
            ds->stagers[cls] = s->next;
            ds->stage_idle -= s->cap;
            ds->stage_busy += s->cap;
            return s;
        }
        // the device's stager streams: created up to STAGE_STREAMS, then shared (a call then may wait for another
        // call's launch on the same stream; calls beyond that many at once would share the few hardware queues anyway)
        if (ds->stage_streams.size() >= STAGE_STREAMS)
            stream = ds->stage_streams[ds->stage_rr++ % STAGE_STREAMS];
    }
    if (stream == nullptr) {
        if (hipStreamCreateWithPriority(&stream, hipStreamNonBlocking, ds->priority) != hipSuccess) {
            // (round 4) a stream that cannot be created now is no reason to fail the call: share an existing one
            (void)hipGetLastError();
            std::lock_guard<std::mutex> lk(ds->mu);
            if (ds->stage_streams.empty()) {
                fail("%s", "staging: stream creation failed");
                return nullptr;
            }
            stream = ds->stage_streams[ds->stage_rr++ % ds->stage_streams.size()];
        } else {
            std::lock_guard<std::mutex> lk(ds->mu);
            ds->stage_streams.push_back(stream);
        }
    }
    Stager *s = new (std::nothrow) Stager();
    if (s == nullptr) {
        fail("%s", "out of memory");
        return nullptr;
    }
    s->stream = stream;
    s->cap = (size_t)4096 << cls;
    s->cls = cls;
    // Fine-grained (coherent) pinned memory: kernels read the staged input and write the results in place over PCIe,
    // and the host rewrites the same bytes for the next call right after it sees the completion words. Coarse-grained
    // host memory (hipHostMallocDefault under HIP_HOST_COHERENT=0) may be cached in the GPU's L2, where a later
    // kernel on this buffer can read lines of the previous call's input.
    const unsigned hflags = ds->stage_coherent ? hipHostMallocCoherent : hipHostMallocDefault;
    if (hipHostMalloc((void **)&s->h, s->cap, hflags) != hipSuccess) {
        // (round 4) the pinned memory of idle buffers of other sizes is what this one may need: free this device's
        // (not every device's -- hipHostFree synchronises the device it frees for), try again
        (void)hipGetLastError();
        release_idle_stagers(ds);
        if (hipHostMalloc((void **)&s->h, s->cap, hflags) != hipSuccess) {
            (void)hipGetLastError();
            delete s;
            fail("%s", "staging: pinned host allocation failed");
            return nullptr;
        }
    }
    if (ds->force_copy || hipHostGetDevicePointer((void **)&s->h_dev, s->h, 0) != hipSuccess) {
        (void)hipGetLastError();  // (handled: the copy path)
        s->h_dev = nullptr;
    }
    if (s->h_dev == nullptr && hipMalloc((void **)&s->d, s->cap) != hipSuccess) {
        (void)hipHostFree(s->h);
        delete s;
        fail("%s", "staging: device allocation failed");
        return nullptr;
    }
    std::lock_guard<std::mutex> lk(ds->mu);
    ds->stage_busy += s->cap;
    return s;
}

// back to the pool after its call (nothing of the call is still queued on its stream); a buffer beyond the pool's bounds
// (above STAGE_KEEP_MAX, or with the idle pool full) is freed instead
static void stager_put(DeviceState *ds, Stager *s)
{
    {
        std::lock_guard<std::mutex> lk(ds->mu);
        ds->stage_busy -= s->cap;
        if (s->cap <= STAGE_KEEP_MAX && ds->stage_idle + s->cap <= ds->stage_pool_cap) {
            s->next = ds->stagers[s->cls];
            ds->stagers[s->cls] = s;
            ds->stage_idle += s->cap;
            return;
        }
    }
    stager_destroy(s);
}

// a lone record's launch publishes a completion word the host polls (roundtrip) for this long
#define PERREC_FLAG_SPIN_US 2000  // + 0.5 us per staged KiB: long records (the span path) poll to their end too

// PTLS_MI355X_COMBINE_STATS=1: per-record launches, calls and the host time of run_calls, printed at exit (tools/gpu_mt.sh)
static struct CombineStats {
    std::atomic<uint64_t> launches{0}, calls{0}, ns{0}, wait_ns{0};
    bool on = getenv("PTLS_MI355X_COMBINE_STATS") != nullptr;
    ~CombineStats()
    {
        if (on && launches.load() != 0)
            fprintf(stderr, "combine stats: %llu launches, %llu calls (%.2f per launch), %.1f us per launch in run_calls, %.1f us of it waiting\n",
                    (unsigned long long)launches.load(), (unsigned long long)calls.load(), (double)calls.load() / (double)launches.load(),
                    (double)ns.load() / 1e3 / (double)launches.load(), (double)wait_ns.load() / 1e3 / (double)launches.load());
    }
} g_cstats;

// ---- the synchronous host-buffer helpers (the per-record picotls path)
//
// One call = a staging buffer and its stream from the device pool, a host copy of the inputs into it, launches whose
// kernels read and write the pinned buffer in place over PCIe (or, where it cannot be mapped, an H2D copy before and a
// D2H copy after), a wait for that stream only, a host copy of the results, and the staged bytes cleared.
// Measured against copying (tools/latency.py, interleaved): 16 B 29 -> 26 us, 1200 B 31 -> 29, 16 KiB 52 -> 38,
// 4 MiB 1.70 -> 1.58 ms.
struct StageCall {
    DeviceState *ds;
    Stager *st = nullptr;
    size_t total = 0;
    size_t clear_lo = 0, clear_hi = SIZE_MAX;  // the staged bytes that held plaintext (all unless narrowed)
    StageCall(DeviceState *d) : ds(d) {}
    ~StageCall()
    {
        if (st != nullptr) {
            // staged plaintext does not outlive the call (with it gone, the ciphertext beside it reveals nothing)
            const size_t hi = clear_hi < total ? clear_hi : total;
            if (hi > clear_lo)
                memset(st->h + clear_lo, 0, hi - clear_lo);
            stager_put(ds, st);
        }
    }
    int acquire(size_t bytes)
    {
        total = bytes;
        return (st = stager_get(ds, bytes)) != nullptr ? 0 : -1;
    }
    uint8_t *host() const { return st->h; }
    uint8_t *dev() const { return st->h_dev != nullptr ? st->h_dev : st->d; }
    hipStream_t stream() const { return st->stream; }
    // runs launch() on the staged buffer: H2D of [0, up) before and D2H of [up, total) after on the copy path; then waits
    // flag_off (mapped staging only, 0: none): nflags words, one per workgroup of the launch's last kernel, that it sets
    // once its results are written (BatchArgs::done_flag); the call returns when it sees them all, without the
    // stream's completion signal (the next user of this stager's stream is ordered after the kernel anyway). After
    // PERREC_FLAG_SPIN_US (+ 0.5 us per staged KiB) without them (a launch queued behind others) the call waits for the
    // stream as usual.
    bool mapped() const { return st->h_dev != nullptr; }
    template <typename Launch>
    int roundtrip(size_t up, Launch launch, size_t flag_off = 0, size_t nflags = 0, u32 token = 0)
    {
        const bool copy = st->h_dev == nullptr;
        if (copy)
            HIP_TRY(hipMemcpyAsync(st->d, st->h, up, hipMemcpyHostToDevice, st->stream));
        LAUNCH_CLEAR();  // (the launches below are checked with hipGetLastError)
        if (launch() != 0) {
            // a kernel of this call may already be queued (the span launch before its combine, the GCM launch before
            // the header-protection one): the buffer is cleared and reused only once nothing of it is in flight
            (void)hipStreamSynchronize(st->stream);
            return -1;
        }
        if (copy)
            HIP_TRY(hipMemcpyAsync(st->h + up, st->d + up, total - up, hipMemcpyDeviceToHost, st->stream));
        const auto t0 = std::chrono::steady_clock::now();
        if (flag_off != 0 && token != 0 && !copy) {
            const u32 *flag = (const u32 *)(st->h + flag_off);
            size_t seen = 0;  // flags [0, seen) are set
            for (unsigned k = 0;; ++k) {
                while (seen < nflags && __atomic_load_n(flag + seen, __ATOMIC_ACQUIRE) == token)
                    ++seen;
                if (seen == nflags) {
                    if (g_cstats.on)
                        g_cstats.wait_ns += (uint64_t)std::chrono::duration_cast<std::chrono::nanoseconds>(std::chrono::steady_clock::now() - t0).count();
                    return 0;
                }
                __builtin_ia32_pause();
                if ((k & 255) == 255 &&
                    std::chrono::steady_clock::now() - t0 > std::chrono::microseconds(PERREC_FLAG_SPIN_US + (int64_t)(total >> 11)))
                    break;
            }
        }
        HIP_TRY(hipStreamSynchronize(st->stream));
        if (g_cstats.on)
            g_cstats.wait_ns += (uint64_t)std::chrono::duration_cast<std::chrono::nanoseconds>(std::chrono::steady_clock::now() - t0).count();
        return 0;
    }
};

// completion tokens of per-record calls (StageCall::roundtrip): process-wide, nonzero, and consecutive calls on one
// staging buffer never share one
static std::atomic<u32> g_done_token{0};
static u32 next_done_token(void)
{
    u32 t;
    while ((t = g_done_token.fetch_add(1, std::memory_order_relaxed) + 1) == 0) {
    }
    return t;
}

static unsigned aux_grid(size_t n, int ncu)
{
    u64 grid = (n + 255) / 256;
    return (unsigned)(grid > (u64)ncu * 4 ? (u64)ncu * 4 : grid);
}

// ---- run-time values to template arguments: f is a generic lambda that takes them as std::integral_constant objects
// (usable as template arguments as they are); the first arm written is the first instantiated
template <auto A, auto B, typename F>
static void with_either(decltype(A) v, F f)  // A when v is A, else B
{
    if (v == A)
        f(std::integral_constant<decltype(A), A>{});
    else
        f(std::integral_constant<decltype(A), B>{});
}

template <typename F>
static void with_bool(bool b, F f) { with_either<true, false>(b, f); }

template <typename F>
static void with_nr(int nr, F f) { with_either<10, 14>(nr, f); }  // AES rounds: 10 (AES-128), else 14 (AES-256)

template <typename F>
static void with_nr_open(int nr, bool open, F f)
{
    with_nr(nr, [&](auto NR) { with_bool(open, [&](auto OPEN) { f(NR, OPEN); }); });
}

// ---- argument checks and copies both families' C ABIs share (`what`: the caller's message prefix)
// keyset_update's index list: every index below nkeys, none listed twice
static int check_update_indices(const char *what, const uint32_t *key_idx, size_t n, size_t nkeys)
{
    std::vector<bool> seen(n != 0 ? nkeys : 0);
    for (size_t i = 0; i < n; ++i) {
        if (key_idx[i] >= nkeys)
            return fail("%s: key index out of range", what);
        if (seen[key_idx[i]])
            return fail("%s: key index listed twice", what);
        seen[key_idx[i]] = true;
    }
    return 0;
}

// a per-record call's arguments (key_ok: the keyset is there and holds the key index)
static int check_single_args(const char *what, bool key_ok, const void *aad, size_t aadlen, const void *output, size_t len)
{
    if (!key_ok || (aadlen != 0 && aad == NULL) || (len != 0 && output == NULL))
        return fail("%s: invalid arguments", what);
    if (len > PTLS_MI355X_MAX_RECORD_LEN || aadlen > PTLS_MI355X_MAX_AAD_LEN)
        return fail("%s: record or AAD longer than PTLS_MI355X_MAX_RECORD_LEN / PTLS_MI355X_MAX_AAD_LEN", what);
    return 0;
}

// ---- calls on two keysets of one family (QUIC packets: `ks` holds the AEAD keys, `hp_ks` the header-protection keys;
// they may be one object). KS has `mu`, `uses`, `ds` and `device`.
// Both keysets' mutexes, two distinct ones taken in the order of their addresses, whichever role each has in the call
template <typename KS>
struct PairLock {
    std::unique_lock<std::mutex> ks_lock, hp_lock;  // (hp_lock: empty when hp_ks is ks)
    PairLock(KS *ks, KS *hp_ks) : ks_lock(ks->mu, std::defer_lock)
    {
        if (hp_ks != ks)
            hp_lock = std::unique_lock<std::mutex>(hp_ks->mu, std::defer_lock);
        const bool ks_first = hp_ks == ks || std::less<KS *>()(ks, hp_ks);
        if (ks_first)
            ks_lock.lock();
        if (hp_ks != ks)
            hp_lock.lock();
        if (!ks_first)
            ks_lock.lock();
    }
};

// `launch()` on `s` as a use of both keysets (both mutexes held): a free or rekey of either orders itself behind it
template <typename KS, typename Launch>
static int launch_and_note_both(KS *ks, KS *hp_ks, hipStream_t s, Launch launch)
{
    const auto on_ks = [&] { return launch_and_note(ks->uses, ks->ds, s, launch); };
    return hp_ks != ks ? launch_and_note(hp_ks->uses, hp_ks->ds, s, on_ks) : on_ks();
}

// a QUIC packet call's arguments (results: the open's only)
template <typename KS>
static int check_quic_args(const char *what, const KS *ks, const KS *hp_ks, bool open, const void *recs, size_t nrecs,
                           const void *in, const void *out, const void *ok, const void *results)
{
    if (ks == NULL || hp_ks == NULL ||
        (nrecs != 0 && (recs == NULL || in == NULL || out == NULL || (open && (ok == NULL || results == NULL)))))
        return fail("%s: invalid arguments", what);
    if (hp_ks->device != ks->device)
        return fail("%s: hp_ks is on another device than ks", what);
    return 0;
}

// a per-record call's input, gathered into its staging buffer
static void gather_iovec(uint8_t *dst, const ptls_mi355x_iovec_t *vec, size_t incnt)
{
    for (size_t v = 0; v < incnt; dst += vec[v].len, ++v)
        if (vec[v].len != 0)
            memcpy(dst, vec[v].base, vec[v].len);
}

#endif  // PTLS_MI355X_HOST_RUNTIME_H
