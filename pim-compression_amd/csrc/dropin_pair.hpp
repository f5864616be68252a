// dropin_pair.hpp -- snappy_compress_gpu / snappy_decompress_gpu on host buffers (reference L2 signatures), included at
// the end of snappy_hip.hip.  Where the bytes go is csrc/dropin_plan.hpp; this file only issues the HIP work.

namespace {   // (C++ linkage: an unnamed namespace inside extern "C" would still export unmangled names)

// The compress pipeline keeps six streams busy at once (copy-in, two K1 launches, the LDS-table helper, framing,
// copy-out).  The HIP runtime multiplexes streams onto GPU_MAX_HW_QUEUES hardware queues (default 4), and two streams on
// one queue run in enqueue order: measured here, the copy-in of chunk k+1 then waits for the K1 launch of chunk k and the
// pipeline degenerates to the phased form (38 instead of 52 GB/s on a 3 GiB input).  The library does NOT touch the
// process environment: a host program that wants the overlap exports GPU_MAX_HW_QUEUES=8 before its first HIP call (the
// CLI and the Python binding do); without it only the overlap is lost, never bytes.

// Streams of one shard's pipeline.  Creating a stream costs milliseconds (a hardware queue each), so the sets are made
// once per process and shard index and kept: a long-lived caller pays for them in its first call only.
struct PipelineStreams {
    hipStream_t in = nullptr, run = nullptr, run2 = nullptr, post = nullptr, out = nullptr;
    hipEvent_t start = nullptr;
    uint64_t* h_len = nullptr;          // page-locked scratch: stream length per chunk / block offsets
    size_t h_len_count = 0;
};

// The cached streams and their page-locked scratch are per process, so overlapped calls from several host threads take
// turns (the reference's entry points are single-threaded and synchronous anyway, snappy_compress.c:618).
std::mutex* pipeline_mutex()
{
    static std::mutex* m = new std::mutex;
    return m;
}

// Cached per (device, shard): streams, events and the DMA queues behind them belong to the device they were created on, and
// the shard-to-device mapping follows the caller's current device (ShardDevices), so shard g of one call and shard g of the
// next may run on different devices; two shards on ONE device (SNAPPY_HIP_OVERSUBSCRIBE) run in different host threads at
// the same time and must not share a set either.
int pipeline_streams(int device, int shard, size_t chunks, PipelineStreams* out)
{
    static std::map<int, PipelineStreams*> cache;
    static std::mutex cache_mutex;
    if (shard < 0 || shard >= 64 || device < 0 || device >= 64) return fail(SNAPPY_HIP_ERR_ARG, "shard / device index out of range");
    PipelineStreams* pp = nullptr;
    {
        std::lock_guard<std::mutex> lock(cache_mutex);
        PipelineStreams*& slot = cache[pipeline_stream_key(device, shard)];
        if (!slot) slot = new PipelineStreams;               // never destroyed (threads may outlive statics)
        pp = slot;
    }
    PipelineStreams& p = *pp;                            // one (device, shard) is only ever touched by the host thread driving that shard
    if (!p.in) {
        HIP_TRY(hipStreamCreateWithFlags(&p.in, hipStreamNonBlocking));
        HIP_TRY(hipStreamCreateWithFlags(&p.run, hipStreamNonBlocking));
        HIP_TRY(hipStreamCreateWithFlags(&p.run2, hipStreamNonBlocking));
        HIP_TRY(hipStreamCreateWithFlags(&p.post, hipStreamNonBlocking));
        HIP_TRY(hipStreamCreateWithFlags(&p.out, hipStreamNonBlocking));
        HIP_TRY(hipEventCreate(&p.start));
        // a stream gets its hardware queue at first use: use each one now, in the load phase, not under the first chunk
        for (hipStream_t st : {p.in, p.run, p.run2, p.post, p.out}) {
            WorkCounter c;
            if (int rc = next_work_counter(&c, st)) return rc;
            if (int rc = work_counter_launched(c, st)) return rc;
        }
        // ... and the first asynchronous copy in either direction on a stream starts a DMA queue of its own (~8 ms)
        const size_t n = 256u << 10;
        void *h = nullptr, *d = nullptr;
        HIP_TRY(hipHostMalloc(&h, n, hipHostMallocPortable));
        HIP_TRY(hipMalloc(&d, n));
        memset(h, 0, n);
        HIP_TRY(hipMemcpyAsync(d, h, n, hipMemcpyHostToDevice, p.in));
        HIP_TRY(hipStreamSynchronize(p.in));
        for (hipStream_t st : {p.out, p.post, p.run, p.run2}) HIP_TRY(hipMemcpyAsync(h, d, n, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipDeviceSynchronize());
        (void)hipFree(d);
        (void)hipHostFree(h);
    }
    if (chunks > p.h_len_count) {
        if (p.h_len) (void)hipHostFree(p.h_len);
        p.h_len = nullptr;
        p.h_len_count = 0;
        const size_t want = std::max<size_t>(chunks, 64);
        HIP_TRY(hipHostMalloc((void**)&p.h_len, want * sizeof(uint64_t), hipHostMallocPortable));
        p.h_len_count = want;
    }
    *out = p;
    return 0;
}

// A shard of either direction: its range, streams and timings, and what it holds on its device -- allocations and
// per-chunk events, recorded as they are made and given back by release().
struct ShardBase : dropin_plan::Range {
    ShardBase(const dropin_plan::Range& r) : dropin_plan::Range(r) {}
    PipelineStreams ps;
    float kernel_ms = 0.f, exposed_in_ms = 0.f;
    std::vector<void*> mem;
    std::vector<hipEvent_t> events;

    template <class T>
    hipError_t alloc(T** p, uint64_t bytes)
    {
        const hipError_t e = hipMalloc((void**)p, bytes);
        if (e == hipSuccess) mem.push_back(*p);
        return e;
    }
    hipError_t event(hipEvent_t* ev)
    {
        const hipError_t e = hipEventCreate(ev);
        if (e == hipSuccess) events.push_back(*ev);
        return e;
    }
    // device memory and per-chunk events (the cached streams stay); safe to call twice
    void release()
    {
        for (hipEvent_t e : events) (void)hipEventDestroy(e);
        for (void* p : mem) (void)hipFree(p);
        events.clear();
        mem.clear();
    }
};

struct CompressChunk : dropin_plan::CompressChunk {
    CompressChunk(const dropin_plan::CompressChunk& p) : dropin_plan::CompressChunk(p) {}
    uint64_t stream_len = 0, out_off = 0;       // this chunk's framed stream, and where its blocks go in the output
    hipEvent_t ev_in = nullptr, ev_k1 = nullptr, ev_run = nullptr;
};

struct CompressShard : ShardBase {
    using ShardBase::ShardBase;
    uint8_t *d_in = nullptr, *d_slots = nullptr, *d_stream = nullptr, *d_offsets = nullptr;    // (d_stream, d_offsets: the pools)
    uint32_t* d_bytes = nullptr;
    uint64_t* d_stream_len = nullptr;
    void* d_scratch[2] = {};                    // one per K1 stream
    uint64_t scratch_bytes = 0;                 // sized for this shard's device
    std::vector<CompressChunk> chunks;          // one chunk = the phased form
};

struct DecompressChunk : dropin_plan::Range {
    DecompressChunk(const dropin_plan::Range& r) : dropin_plan::Range(r) {}
    hipEvent_t ev_in = nullptr, ev_run = nullptr;
};

struct DecompressShard : ShardBase {
    using ShardBase::ShardBase;
    uint64_t in_off = 0, in_len = 0;            // slice of the compressed stream (relative to input->buffer)
    uint8_t *d_stream = nullptr, *d_out = nullptr;
    uint64_t* d_boff = nullptr;
    uint32_t* d_status = nullptr;
    bool bad = false, bad_chain = false;
    std::vector<DecompressChunk> chunks;        // one chunk = the phased form
    // size chain of the shard (snappy_decompress.c:317-340), walked on demand: blocks [0, walk.block) have their offsets
    // (relative to in_off) in ps.h_len[], [walk.block] holds the end of the last one; walk.at = its stream position
    dropin_plan::Walk walk;
};

// Error returns leave through this: drain every device a shard used, then give its memory back (the normal path has
// released everything in its timed "free" phase by then, and release() is idempotent).
template <class Shard>
struct ShardCleanup {
    std::vector<Shard>& shards;
    const ShardDevices& devs;
    ~ShardCleanup()
    {
        for (size_t g = 0; g < shards.size(); ++g) {
            if (shards[g].mem.empty() && shards[g].events.empty()) continue;
            if (hipSetDevice(devs.device_of((int)g)) == hipSuccess) (void)hipDeviceSynchronize();
            shards[g].release();
        }
    }
};

// zeroed by every call; `pre` accumulates over a program's calls (dpu_snappy.c:169-192)
void zero_phases(struct program_runtime* rt) { rt->d_alloc = rt->load = rt->copy_in = rt->run = rt->copy_out = rt->d_free = 0.0; }

snappy_status say(const dropin_plan::Verdict& v)
{
    fprintf(stderr, "%s\n", v.message.c_str());
    return v.status;
}

snappy_status no_device()
{
    fprintf(stderr, "snappy_hip: no HIP device available; the -d path has no CPU fallback\n");
    return SNAPPY_INVALID_INPUT;
}

void place(struct host_buffer_context* output, uint64_t n)
{
    output->length = n;
    output->curr = output->buffer + n;
}

snappy_status report(const char* where)
{
    fprintf(stderr, "snappy_hip: %s failed: %s\n", where, g_last_error.c_str());
    return SNAPPY_INVALID_INPUT;   // the reference maps a failed launch to this (snappy_compress.c:618-623)
}

// fn(shard, g) on the device of every non-empty shard (of every shard with `all`), one host thread per shard
template <class Shard, class Fn>
int on_shards(std::vector<Shard>& sh, const ShardDevices& devs, Fn fn, bool all = false)
{
    return for_each_device((int)sh.size(), [&](int g) -> int {
        HIP_TRY(hipSetDevice(devs.device_of(g)));
        return (all || sh[g].num_blocks) ? fn(sh[g], g) : 0;
    });
}

// one timed phase (dpu_alloc / dpu_load / dpu_free): its seconds go to *seconds, a failure becomes report(where)
template <class Shard, class Fn>
snappy_status timed_phase(std::vector<Shard>& sh, const ShardDevices& devs, double* seconds, const char* where, Fn fn, bool all = false)
{
    const double t0 = now_seconds();
    const int rc = on_shards(sh, devs, fn, all);
    *seconds = now_seconds() - t0;
    return rc ? report(where) : SNAPPY_OK;
}

// "load" phase (dpu_load, snappy_compress.c:541): make the device ready so that the copy and run phases measure
// copies and kernels -- code object on the device, copy engines and the co-run helper stream initialised.
int warm_up_device()
{
    hipFuncAttributes fa;
    // (the default K1 launch for blocks of more than 8 KiB: the cached global-table kernel and the LDS-table kernel, stream form)
    HIP_TRY(hipFuncGetAttributes(&fa, reinterpret_cast<const void*>(snappy_hip::compress_blocks_global_table_kernel<64, 3, 1, 512>)));
    HIP_TRY(hipFuncGetAttributes(&fa, reinterpret_cast<const void*>(snappy_hip::compress_blocks_lds_table_kernel<64, 3>)));
    HIP_TRY(hipFuncGetAttributes(&fa, reinterpret_cast<const void*>(snappy_hip::gather_slots_kernel)));
    HIP_TRY(hipFuncGetAttributes(&fa, reinterpret_cast<const void*>(snappy_hip::decompress_blocks_kernel)));
    CoRunResources* cr = nullptr;
    if (int rc = corun_resources(&cr)) return rc;
    WorkCounter c;
    if (int rc = next_work_counter(&c, nullptr)) return rc;      // also touches the module's globals
    uint32_t probe = 0;
    HIP_TRY(hipMemcpy(&probe, c.ptr, sizeof(probe), hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(c.ptr, &probe, sizeof(probe), hipMemcpyHostToDevice));
    if (int rc = work_counter_launched(c, nullptr)) return rc;
    // the first copy of more than a few KiB in either direction starts the DMA engines (~8 ms, once per process)
    static std::mutex engines_mutex;
    static bool engines_started[64] = {};                        // per process and device, not per (short-lived) shard thread
    int dev = 0;
    HIP_TRY(hipGetDevice(&dev));
    std::lock_guard<std::mutex> engines_lock(engines_mutex);
    if (dev >= 0 && dev < 64 && !engines_started[dev]) {
        const size_t n = 1u << 20;
        void *h = nullptr, *d = nullptr;
        HIP_TRY(hipHostMalloc(&h, n, hipHostMallocPortable));
        HIP_TRY(hipMalloc(&d, n));
        memset(h, 0, n);
        HIP_TRY(hipMemcpy(d, h, n, hipMemcpyHostToDevice));
        HIP_TRY(hipMemcpy(h, d, n, hipMemcpyDeviceToHost));
        (void)hipFree(d);
        (void)hipHostFree(h);
        engines_started[dev] = true;
    }
    HIP_TRY(hipDeviceSynchronize());
    return 0;
}

// The end of either direction.  copy_in / run = the slowest shard's exposed copy-in and kernel time (the shards run side
// by side); copy_out = the rest of the section's wall time.  Then the per-tasklet log lines (dpu-compress/dpu_task.c:88)
// and the timed free (dpu_free, :707).
template <class Shard, class InBytes>
snappy_status finish_shards(std::vector<Shard>& sh, const ShardDevices& devs, struct program_runtime* runtime, double wall,
                            InBytes in_bytes)
{
    float in_ms = 0.f, run_ms = 0.f;
    for (const Shard& s : sh) {
        in_ms = std::max(in_ms, s.exposed_in_ms);
        run_ms = std::max(run_ms, s.kernel_ms);
    }
    runtime->copy_in = in_ms / 1000.0;
    runtime->run = run_ms / 1000.0;
    runtime->copy_out = std::max(0.0, wall - runtime->copy_in - runtime->run);
    for (size_t g = 0; g < sh.size(); ++g)
        printf("GPU %d: %f s, %lu bytes\n", (int)g, sh[g].kernel_ms / 1000.0, (unsigned long)in_bytes(sh[g]));
    return timed_phase(sh, devs, &runtime->d_free, "free", [](Shard& s, int) -> int {
        s.release();
        return 0;
    });
}

// The drop-in pair's device side (phases of snappy_compress.c:528-709 / snappy_decompress.c:306-493), overlapped per
// chunk k+1 is copied in while chunk k is compressed / decoded and chunk k-1 is framed and
// copied out, on separate streams; one chunk per shard IS the reference's phased order.  Chunks are whole blocks and the
// host concatenates chunk streams like per-device streams, so the bytes do not depend on the chunking.  The enqueue order
// (kernels of k, copy-in of k+1, copy-out of k-1) keeps the overlap when the caller's buffers are pageable and
// hipMemcpyAsync degrades to a blocking staged copy.  program_runtime holds the EXPOSED parts: copy_in = until the first
// chunk is on the device, run = from there to the last kernel, copy_out = the rest of the wall time.
snappy_status compress_gpu_body(struct host_buffer_context* input, struct host_buffer_context* output, uint32_t block_size,
                                struct program_runtime* runtime)
{
    double t0 = now_seconds();
    if (!input || !output || !runtime) return SNAPPY_INVALID_INPUT;
    if (input->length && !input->buffer) return SNAPPY_INVALID_INPUT;
    zero_phases(runtime);
    if (!block_size_ok(block_size)) return say(dropin_plan::bad_block_size(block_size, ""));
    if (input->length > 0xffffffffull) {
        fprintf(stderr, "snappy_hip: input of %lu bytes does not fit the format's uint32 length\n", input->length);
        return SNAPPY_BUFFER_TOO_SMALL;
    }
    const uint64_t n = input->length;
    const uint64_t nb = snappy_hip_num_blocks(n, block_size);
    const ShardDevices devs = requested_devices();
    if (devs.shards <= 0) return no_device();
    const int gpus = dropin_plan::shard_count(devs.shards, nb);
    const std::vector<dropin_plan::Range> part = dropin_plan::partition(nb, gpus, n, block_size);
    std::vector<CompressShard> sh(part.begin(), part.end());
    ShardCleanup<CompressShard> cleanup{sh, devs};
    uint8_t hdr[10];
    const uint32_t hdr_len = snappy_hip_write_header(hdr, (uint32_t)n, block_size);   // :523-525
    const uint32_t stride = snappy_hip_slot_stride(block_size);
    runtime->pre += now_seconds() - t0;
    // One code path: a shard is a list of chunks; SNAPPY_HIP_PIPELINE_BLOCKS=0 (or a small shard) makes it one chunk, which
    // is the strictly phased copy-in / run / copy-out of the reference (snappy_compress.c:547-704).
    const uint64_t per = dropin_plan::shard_blocks(nb, gpus);
    const uint64_t chunk_blocks =
        dropin_plan::compress_chunk_blocks(per, dropin_plan::pipeline_chunk_blocks(per, block_size, getenv("SNAPPY_HIP_PIPELINE_BLOCKS")));

    // alloc (dpu_alloc, snappy_compress.c:535)
    snappy_status st = timed_phase(sh, devs, &runtime->d_alloc, "device allocation", [&](CompressShard& s, int) -> int {
        const dropin_plan::CompressLayout l = dropin_plan::compress_layout(s.num_blocks, s.plain_len, block_size, stride, chunk_blocks);
        s.chunks.assign(l.chunks.begin(), l.chunks.end());
        s.scratch_bytes = snappy_hip_compress_scratch_bytes();          // for THIS device: its CU count sizes the scratch
        HIP_TRY(s.alloc(&s.d_in, s.plain_len + 16));
        HIP_TRY(s.alloc(&s.d_slots, s.num_blocks * (uint64_t)stride));
        HIP_TRY(s.alloc(&s.d_bytes, s.num_blocks * sizeof(uint32_t)));
        HIP_TRY(s.alloc(&s.d_offsets, l.offsets_pool));
        HIP_TRY(s.alloc(&s.d_stream_len, dropin_plan::pad256(s.chunks.size() * sizeof(uint64_t))));
        HIP_TRY(s.alloc(&s.d_stream, l.stream_pool));
        for (size_t i = 0; i < std::min<size_t>(2, s.chunks.size()); ++i) HIP_TRY(s.alloc(&s.d_scratch[i], s.scratch_bytes));
        for (CompressChunk& c : s.chunks)
            for (hipEvent_t* e : {&c.ev_in, &c.ev_k1, &c.ev_run}) HIP_TRY(s.event(e));
        return 0;
    });
    if (st) return st;

    // load (dpu_load, :541): code object, copy engines, and this shard's streams with their hardware queues
    st = timed_phase(sh, devs, &runtime->load, "code object load", [&](CompressShard& s, int g) -> int {
        if (int r = warm_up_device()) return r;
        return s.num_blocks ? pipeline_streams(devs.device_of(g), g, s.chunks.size(), &s.ps) : 0;
    }, true);
    if (st) return st;

    // the output buffer: the caller's (finite max) or ours, grown when a chunk does not fit
    const bool caller_owned = output->buffer && output->max != ~0UL;
    uint64_t capacity = caller_owned ? output->max : 0;
    if (!caller_owned) {
        capacity = 32 + input->length + input->length / 6;      // the reference's own bound (snappy_compress.c:446-449)
        uint8_t* nbuf = (uint8_t*)realloc(output->buffer, capacity);
        if (!nbuf) {
            fprintf(stderr, "snappy_hip: cannot allocate %lu bytes for the output\n", (unsigned long)capacity);
            return SNAPPY_BUFFER_TOO_SMALL;
        }
        output->buffer = nbuf;
    }
    if (capacity < hdr_len) {
        fprintf(stderr, "snappy_hip: output buffer of %lu bytes cannot hold the stream header\n", (unsigned long)capacity);
        return SNAPPY_BUFFER_TOO_SMALL;
    }
    memcpy(output->buffer, hdr, hdr_len);
    uint64_t total = hdr_len;
    bool too_small = false;
    // place chunk c of shard s at `total` and start its copy-out
    auto copy_out_chunk = [&](CompressShard& s, CompressChunk& c) -> int {
        const uint64_t body = c.stream_len - c.local_hdr;
        c.out_off = total;
        if (total + body > capacity) {
            if (caller_owned) {
                too_small = true;
                total += body;
                return 0;
            }
            // copies into the old buffer must land before it moves: every shard's copy-out stream, each on its own device
            // (this runs either on shard 0's thread inside the pipeline or on the caller's thread after the join)
            int here = 0;
            HIP_TRY(hipGetDevice(&here));
            for (size_t g2 = 0; g2 < sh.size(); ++g2) {
                if (!sh[g2].num_blocks || !sh[g2].ps.out) continue;
                HIP_TRY(hipSetDevice(devs.device_of((int)g2)));
                HIP_TRY(hipStreamSynchronize(sh[g2].ps.out));
            }
            HIP_TRY(hipSetDevice(here));
            capacity = std::max(total + body, capacity + capacity / 2);
            uint8_t* nbuf = (uint8_t*)realloc(output->buffer, capacity);
            if (!nbuf) return fail(SNAPPY_HIP_ERR_RUNTIME, "cannot grow the output buffer");
            output->buffer = nbuf;
        }
        if (!too_small)
            HIP_TRY(hipMemcpyAsync(output->buffer + c.out_off, s.d_stream + c.stream_at + c.local_hdr, body, hipMemcpyDeviceToHost,
                                   s.ps.out));
        total += body;
        return 0;
    };

    // the pipeline (:547-704).  Shard 0 knows where its output goes and copies out as it runs; later shards learn their
    // place once every earlier shard has reported its lengths, and copy out after the join.
    t0 = now_seconds();
    int rc = on_shards(sh, devs, [&](CompressShard& s, int g) -> int {
        const size_t n = s.chunks.size();
        auto copy_in = [&](size_t k) -> int {
            CompressChunk& c = s.chunks[k];
            HIP_TRY(hipMemcpyAsync(s.d_in + c.plain_off, input->buffer + s.plain_off + c.plain_off, c.plain_len, hipMemcpyHostToDevice,
                                   s.ps.in));
            HIP_TRY(hipEventRecord(c.ev_in, s.ps.in));
            return 0;
        };
        auto finish = [&](size_t k) -> int {
            CompressChunk& c = s.chunks[k];
            HIP_TRY(hipEventSynchronize(c.ev_run));
            c.stream_len = s.ps.h_len[k];
            return g == 0 ? copy_out_chunk(s, c) : 0;
        };
        HIP_TRY(hipEventRecord(s.ps.start, s.ps.in));
        if (int r = copy_in(0)) return r;
        for (size_t k = 0; k < n; ++k) {
            CompressChunk& c = s.chunks[k];
            uint8_t* slots = s.d_slots + c.first_block * (uint64_t)stride;
            // Two launches in flight, on alternating streams with a hash-table scratch each: a launch of one block per
            // wavefront ends in a tail of half-empty CUs, which the next chunk's wavefronts fill.
            hipStream_t run = (k & 1) ? s.ps.run2 : s.ps.run;
            HIP_TRY(hipStreamWaitEvent(run, c.ev_in, 0));
            int r = snappy_hip_compress_blocks(s.d_in + c.plain_off, c.plain_len, block_size, slots, stride, s.d_bytes + c.first_block,
                                               s.d_scratch[k & 1], s.scratch_bytes, run);
            if (r) return r;
            // scan + gather on a stream of their own: small kernels that crawl beside the next chunk's K1 must not
            // hold back the K1 launch after that
            HIP_TRY(hipEventRecord(c.ev_k1, run));
            HIP_TRY(hipStreamWaitEvent(s.ps.post, c.ev_k1, 0));
            r = snappy_hip_compact(slots, stride, s.d_bytes + c.first_block, c.plain_len, block_size, s.d_stream + c.stream_at,
                                   (uint64_t*)(s.d_offsets + c.offsets_at), s.d_stream_len + k, s.ps.post);
            if (r) return r;
            HIP_TRY(hipMemcpyAsync(&s.ps.h_len[k], s.d_stream_len + k, sizeof(uint64_t), hipMemcpyDeviceToHost, s.ps.post));
            HIP_TRY(hipEventRecord(c.ev_run, s.ps.post));
            if (k + 1 < n)
                if (int r2 = copy_in(k + 1)) return r2;
            if (k >= 1)
                if (int r2 = finish(k - 1)) return r2;
        }
        if (int r = finish(n - 1)) return r;
        HIP_TRY(hipStreamSynchronize(s.ps.out));
        HIP_TRY(hipEventElapsedTime(&s.exposed_in_ms, s.ps.start, s.chunks[0].ev_in));
        HIP_TRY(hipEventElapsedTime(&s.kernel_ms, s.chunks[0].ev_in, s.chunks[n - 1].ev_run));
        if (env_int("SNAPPY_HIP_PIPELINE_TRACE", 0))
            for (size_t k = 0; k < n; ++k) {
                float a = 0.f, b = 0.f, c = 0.f;
                HIP_TRY(hipEventElapsedTime(&a, s.ps.start, s.chunks[k].ev_in));
                HIP_TRY(hipEventElapsedTime(&b, s.ps.start, s.chunks[k].ev_k1));
                HIP_TRY(hipEventElapsedTime(&c, s.ps.start, s.chunks[k].ev_run));
                fprintf(stderr, "chunk %zu: copied in at %.2f ms, compressed at %.2f ms, framed at %.2f ms\n", k, a, b, c);
            }
        if (n >= 2) {                                   // the second-to-last launch runs on the other stream and may end later
            float other = 0.f;
            HIP_TRY(hipEventElapsedTime(&other, s.chunks[0].ev_in, s.chunks[n - 2].ev_run));
            s.kernel_ms = std::max(s.kernel_ms, other);
        }
        return 0;
    });
    if (rc) return report("compress pipeline");
    if (sh.size() > 1) {
        for (size_t g = 1; g < sh.size() && !rc; ++g) {
            CompressShard& s = sh[g];
            if (!s.num_blocks) continue;
            if ((rc = (int)hipSetDevice(devs.device_of((int)g)))) break;
            for (auto& c : s.chunks)
                if ((rc = copy_out_chunk(s, c))) break;
        }
        if (!rc)
            rc = on_shards(sh, devs, [](CompressShard& s, int g) -> int {
                if (g) HIP_TRY(hipStreamSynchronize(s.ps.out));
                return 0;
            });
        if (rc) return report("device-to-host copy");
    }
    st = finish_shards(sh, devs, runtime, now_seconds() - t0, [](const CompressShard& s) { return s.plain_len; });
    if (st) return st;
    if (too_small) {
        fprintf(stderr, "snappy_hip: output buffer of %lu bytes cannot hold the %lu-byte stream\n", (unsigned long)output->max,
                (unsigned long)total);
        return SNAPPY_BUFFER_TOO_SMALL;
    }
    if (!caller_owned) {
        uint8_t* nbuf = (uint8_t*)realloc(output->buffer, total ? total : 1);
        if (nbuf) output->buffer = nbuf;
    }
    place(output, total);
    return SNAPPY_OK;
}

// Decompress counterpart: sizes are known from the host pre-scan, so the whole pipeline is enqueued without a host
// round trip; chunk k's plaintext goes straight into its range of output->buffer (snappy_decompress.c:463).
snappy_status decompress_gpu_body(struct host_buffer_context* input, struct host_buffer_context* output, struct program_runtime* runtime)
{
    double t0 = now_seconds();
    if (!input || !output || !runtime) return SNAPPY_INVALID_INPUT;
    if (!input->buffer || !input->curr || input->curr < input->buffer) return SNAPPY_INVALID_INPUT;
    zero_phases(runtime);

    // block-size varint (snappy_decompress.c:298-303)
    const uint8_t* const buf = input->buffer;
    const uint64_t in_total = input->length;
    uint64_t at = (uint64_t)(input->curr - input->buffer);
    uint32_t bs = 0;
    const uint32_t used = (at <= in_total) ? get_varint32(buf + at, in_total - at, &bs) : 0;
    if (!used) {
        fprintf(stderr, "Failed to read decompressed block size\n");
        return SNAPPY_INVALID_INPUT;
    }
    at += used;
    input->curr += used;
    const uint64_t total = output->length;
    if (total == 0) {
        runtime->pre += now_seconds() - t0;
        return (at == in_total) ? SNAPPY_OK : SNAPPY_INVALID_INPUT;
    }
    if (!block_size_ok(bs)) return say(dropin_plan::bad_block_size(bs, " in the stream"));
    if (!output->buffer) {
        fprintf(stderr, "snappy_hip: output->buffer is NULL (setup_decompression allocates it, snappy_decompress.c:207-209)\n");
        return SNAPPY_INVALID_INPUT;
    }
    const uint64_t nb = snappy_hip_num_blocks(total, bs);
    // the header is untrusted: every block needs at least its u32 size prefix, so a stream of in_total - at bytes cannot
    // hold more than (in_total - at) / 4 blocks -- checked before anything is sized by nb
    if (nb > (in_total - at) / 4) {
        fprintf(stderr, "snappy_hip: header promises %lu blocks, the stream has room for %lu\n", (unsigned long)nb,
                (unsigned long)((in_total - at) / 4));
        return SNAPPY_INVALID_INPUT;
    }
    const ShardDevices devs = requested_devices();
    if (devs.shards <= 0) return no_device();
    const int gpus = dropin_plan::shard_count(devs.shards, nb);
    const uint64_t per = dropin_plan::shard_blocks(nb, gpus);
    const dropin_plan::DecompressChunking plan = dropin_plan::decompress_chunking(
        per, dropin_plan::pipeline_chunk_blocks(per, bs, getenv("SNAPPY_HIP_PIPELINE_BLOCKS")), gpus);
    const std::vector<dropin_plan::Range> part = dropin_plan::partition(nb, gpus, total, bs);
    std::vector<DecompressShard> sh(part.begin(), part.end());
    ShardCleanup<DecompressShard> cleanup{sh, devs};
    std::vector<uint64_t> off;          // every block's stream offset, unless the one shard walks the chain in its pipeline
    if (plan.walk_in_pipeline) {
        sh[0].in_off = at;
        sh[0].in_len = in_total - at;
    } else {
        // host pre-scan of the size chain (:306-341): every offset is needed before the blocks are split over devices.  In
        // parallel shares where the stream is long enough (csrc/host_chain.hpp; the serial chase costs ~7 ms per GiB, all
        // of `pre`); SNAPPY_HIP_HOST_WALK_THREADS=1 is the serial walk alone, which also names a damaged stream's fault.
        const unsigned walk_threads = (unsigned)std::max(1, env_int("SNAPPY_HIP_HOST_WALK_THREADS",
                                                                   (int)std::min(16u, std::max(1u, std::thread::hardware_concurrency()))));
        if (!host_chain::parallel_walk(buf, in_total, at, nb, bs, walk_threads, off)) {
            off.assign(nb + 1, 0);
            const dropin_plan::Walk w = dropin_plan::walk_chain(buf, in_total, 0, off.data(), {0, at}, nb);
            const std::string err = dropin_plan::whole_walk_error(w, nb, in_total);
            if (!err.empty()) {
                fprintf(stderr, "snappy_hip: %s\n", err.c_str());
                return SNAPPY_INVALID_INPUT;
            }
        }
        for (DecompressShard& s : sh) {
            s.in_off = off[s.first_block];
            s.in_len = off[s.first_block + s.num_blocks] - s.in_off;
        }
    }
    runtime->pre += now_seconds() - t0;
    snappy_status st = timed_phase(sh, devs, &runtime->d_alloc, "device allocation", [&](DecompressShard& s, int) -> int {
        const std::vector<dropin_plan::Range> chunks = dropin_plan::split_blocks(s.num_blocks, s.plain_len, bs, plan.chunk_blocks);
        s.chunks.assign(chunks.begin(), chunks.end());
        for (DecompressChunk& c : s.chunks)
            for (hipEvent_t* e : {&c.ev_in, &c.ev_run}) HIP_TRY(s.event(e));
        HIP_TRY(s.alloc(&s.d_stream, s.in_len + 16));
        HIP_TRY(s.alloc(&s.d_boff, s.num_blocks * sizeof(uint64_t)));
        HIP_TRY(s.alloc(&s.d_out, s.plain_len + 16));
        HIP_TRY(s.alloc(&s.d_status, s.num_blocks * sizeof(uint32_t)));
        return 0;
    });
    if (st) return st;

    st = timed_phase(sh, devs, &runtime->load, "code object load", [&](DecompressShard& s, int g) -> int {
        if (int r = warm_up_device()) return r;
        if (!s.num_blocks) return 0;
        if (int r = pipeline_streams(devs.device_of(g), g, s.num_blocks + 1, &s.ps)) return r;   // page-locked home of the block offsets
        s.walk = {0, s.in_off};
        if (!off.empty()) {                                                 // chain already walked, in `pre`
            for (uint64_t i = 0; i <= s.num_blocks; ++i) s.ps.h_len[i] = off[s.first_block + i] - s.in_off;
            s.walk = {s.num_blocks, s.in_off + s.in_len};
        }
        return 0;
    }, true);
    if (st) return st;

    t0 = now_seconds();
    int rc = on_shards(sh, devs, [&](DecompressShard& s, int) -> int {
        const size_t n = s.chunks.size();
        const uint64_t* rel = s.ps.h_len;
        auto copy_out = [&](size_t k) -> int {
            DecompressChunk& c = s.chunks[k];
            HIP_TRY(hipStreamWaitEvent(s.ps.out, c.ev_run, 0));
            HIP_TRY(hipMemcpyAsync(output->buffer + s.plain_off + c.plain_off, s.d_out + c.plain_off, c.plain_len, hipMemcpyDeviceToHost,
                                   s.ps.out));
            return 0;
        };
        HIP_TRY(hipEventRecord(s.ps.start, s.ps.in));
        size_t issued = 0;
        for (size_t k = 0; k < n; ++k) {
            DecompressChunk& c = s.chunks[k];
            // the host walks this chunk's part of the size chain while the previous chunk is still being copied in
            s.walk = dropin_plan::walk_chain(buf, in_total, s.in_off, s.ps.h_len, s.walk, c.first_block + c.num_blocks);
            if (s.walk.stop != dropin_plan::kDone) {
                s.bad_chain = true;
                break;
            }
            const uint64_t in_off = rel[c.first_block], in_len = rel[c.first_block + c.num_blocks] - in_off;   // in the shard's slice
            HIP_TRY(hipMemcpyAsync(s.d_boff + c.first_block, rel + c.first_block, c.num_blocks * sizeof(uint64_t), hipMemcpyHostToDevice,
                                   s.ps.in));
            HIP_TRY(hipMemcpyAsync(s.d_stream + in_off, buf + s.in_off + in_off, in_len, hipMemcpyHostToDevice, s.ps.in));
            HIP_TRY(hipEventRecord(c.ev_in, s.ps.in));
            HIP_TRY(hipStreamWaitEvent(s.ps.run, c.ev_in, 0));
            // block i of the chunk is read at d_stream + d_boff[first + i] (offsets stay relative to the shard's slice)
            int r = snappy_hip_decompress_blocks(s.d_stream, s.in_len, s.d_boff + c.first_block, c.plain_len, bs, s.d_out + c.plain_off,
                                                 s.d_status + c.first_block, s.ps.run);
            if (r) return r;
            HIP_TRY(hipEventRecord(c.ev_run, s.ps.run));
            ++issued;
            if (k >= 1)
                if (int r2 = copy_out(k - 1)) return r2;
        }
        if (!s.bad_chain && s.walk.at != s.in_off + s.in_len) s.bad_chain = true;    // the chain must end where the slice ends
        if (issued && !s.bad_chain)
            if (int r = copy_out(issued - 1)) return r;
        HIP_TRY(hipStreamSynchronize(s.ps.in));
        HIP_TRY(hipStreamSynchronize(s.ps.run));
        HIP_TRY(hipStreamSynchronize(s.ps.out));
        if (s.bad_chain || !issued) return 0;
        std::vector<uint32_t> status(s.num_blocks);
        HIP_TRY(hipMemcpy(status.data(), s.d_status, s.num_blocks * sizeof(uint32_t), hipMemcpyDeviceToHost));
        for (uint64_t i = 0; i < s.num_blocks; ++i)
            if (status[i] != SNAPPY_HIP_BLOCK_OK) s.bad = true;
        HIP_TRY(hipEventElapsedTime(&s.exposed_in_ms, s.ps.start, s.chunks[0].ev_in));
        HIP_TRY(hipEventElapsedTime(&s.kernel_ms, s.chunks[0].ev_in, s.chunks[n - 1].ev_run));
        return 0;
    });
    const double wall = now_seconds() - t0;
    if (rc) return report("decompress pipeline");
    if ((st = finish_shards(sh, devs, runtime, wall, [](const DecompressShard& s) { return s.in_len; }))) return st;
    for (auto& s : sh) {
        if (s.bad_chain) {
            fprintf(stderr, "snappy_hip: size chain leaves the stream (block %lu of %lu)\n",
                    (unsigned long)(s.first_block + s.walk.block), (unsigned long)(s.first_block + s.num_blocks));
            return SNAPPY_INVALID_INPUT;
        }
        if (s.bad) {
            fprintf(stderr, "snappy_hip: malformed block in the stream\n");
            return SNAPPY_INVALID_INPUT;
        }
    }
    output->curr = output->buffer + total;
    return SNAPPY_OK;
}

// ---- The single-device calls (byte-range decode, byte-range overwrite, raw Snappy): no sharding, no overlap. ----

// claims output->buffer for n bytes: the caller's where its max is finite, else (re)allocated here
snappy_status claim_output(struct host_buffer_context* output, uint64_t n)
{
    const bool caller_owned = output->buffer && output->max != ~0UL;
    if (caller_owned && output->max < n) {
        fprintf(stderr, "snappy_hip: output buffer of %lu bytes cannot hold %lu bytes\n", (unsigned long)output->max, (unsigned long)n);
        return SNAPPY_BUFFER_TOO_SMALL;
    }
    if (!caller_owned) {
        uint8_t* nbuf = (uint8_t*)realloc(output->buffer, n ? n : 1);
        if (!nbuf) {
            fprintf(stderr, "snappy_hip: cannot allocate %lu bytes for the output\n", (unsigned long)n);
            return SNAPPY_BUFFER_TOO_SMALL;
        }
        output->buffer = nbuf;
    }
    return SNAPPY_OK;
}

// One phased, synchronous call on the current device, in the reference's own steps (snappy_decompress.c:292-493): host checks
// (`pre`), buffers, load, uploads, one launch, the way back, free -- each timed into its program_runtime field, a failed step
// reported once.  Device memory goes back when the call leaves, however it leaves.
struct PhasedCall {
    struct Want {
        void** p;
        uint64_t bytes;
        template <class T>
        Want(T** p, uint64_t bytes) : p((void**)p), bytes(bytes) {}
    };
    struct Copy {
        void* dst;
        const void* src;
        uint64_t bytes;
    };

    struct program_runtime* const rt;
    const double t0 = now_seconds();
    std::vector<void*> mem;

    explicit PhasedCall(struct program_runtime* runtime) : rt(runtime) { zero_phases(rt); }
    ~PhasedCall() { release(); }
    void release()
    {
        for (void* p : mem) (void)hipFree(p);
        mem.clear();
    }

    // fn's seconds go to *field, its failure (non-zero, g_last_error set) becomes report(where)
    template <class Fn>
    snappy_status phase(double* field, const char* where, Fn fn)
    {
        const double t = now_seconds();
        if (fn()) return report(where);
        *field = now_seconds() - t;
        return SNAPPY_OK;
    }

    // a call that the host alone decides
    snappy_status done_on_host()
    {
        rt->pre += now_seconds() - t0;
        return SNAPPY_OK;
    }
    snappy_status need_device() const { return snappy_hip_device_count() > 0 ? SNAPPY_OK : no_device(); }

    // the end of `pre`: the buffers (dpu_alloc), then the load phase
    snappy_status buffers(std::initializer_list<Want> wants)
    {
        rt->pre += now_seconds() - t0;
        const snappy_status st = phase(&rt->d_alloc, "device allocation", [&]() -> int {
            for (const Want& w : wants) {
                HIP_TRY(hipMalloc(w.p, w.bytes ? w.bytes : 1));
                mem.push_back(*w.p);
            }
            return 0;
        });
        return st ? st : phase(&rt->load, "code object load", warm_up_device);
    }

    static int copy(std::initializer_list<Copy> copies, hipMemcpyKind kind, const char* what)
    {
        for (const Copy& c : copies)
            if (c.bytes && hipMemcpy(c.dst, c.src, c.bytes, kind) != hipSuccess) return fail(SNAPPY_HIP_ERR_RUNTIME, what);
        return 0;
    }
    snappy_status upload(std::initializer_list<Copy> copies)
    {
        return phase(&rt->copy_in, "host-to-device copy", [&] { return copy(copies, hipMemcpyHostToDevice, "hipMemcpy to the device"); });
    }
    // run = launch + synchronize
    template <class Fn>
    snappy_status launch(const char* what, Fn fn)
    {
        return phase(&rt->run, what, [&]() -> int {
            if (int rc = fn()) return rc;
            HIP_TRY(hipDeviceSynchronize());
            return 0;
        });
    }
    // copy_out = fn: download()s, with whatever the call decides between them (its verdict, its output buffer)
    template <class Fn>
    snappy_status copy_out(Fn fn)
    {
        return phase(&rt->copy_out, "device-to-host copy", fn);
    }
    static int download(std::initializer_list<Copy> copies) { return copy(copies, hipMemcpyDeviceToHost, "hipMemcpy to the host"); }
    snappy_status free_buffers()
    {
        return phase(&rt->d_free, "free", [&] {
            release();
            return 0;
        });
    }
};

// One byte range of a framed file (snappy_decompress_range_gpu): the header, the size chain on the host up to the last block
// the range touches, only those blocks' bytes to the device, one range through snappy_hip_decompress_ranges, `length` bytes back.
snappy_status decompress_range_gpu_body(struct host_buffer_context* input, struct host_buffer_context* output, uint64_t offset,
                                        uint64_t length, struct program_runtime* runtime)
{
    if (!input || !output || !runtime || !input->buffer) return SNAPPY_INVALID_INPUT;
    PhasedCall call(runtime);
    const uint8_t* const buf = input->buffer;
    const uint64_t in_total = input->length;
    const dropin_plan::Container c = dropin_plan::open_container(buf, in_total);
    dropin_plan::Span span;
    if (const dropin_plan::Verdict v = dropin_plan::resolve_span(c, offset, length, "range", &span)) return say(v);
    if (snappy_status st = claim_output(output, length)) return st;
    place(output, 0);
    if (length == 0) return call.done_on_host();
    std::vector<uint64_t> off;      // (:317-340), then relative to the first touched block's
    if (const dropin_plan::Verdict v = dropin_plan::walk_to(buf, in_total, c, span.last + 1, false, off)) return say(v);
    const uint64_t in_lo = off[span.first], in_len = off[span.last + 1] - in_lo;
    for (uint64_t b = 0; b <= span.last; ++b) off[b] = b >= span.first ? off[b] - in_lo : 0;
    if (snappy_status st = call.need_device()) return st;
    const uint64_t scratch_bytes =
        snappy_hip::range_prefix_bytes(1) + std::min<uint64_t>(span.blocks, range_grid_cap()) * snappy_hip::range_slot_bytes(c.bs);

    uint8_t *d_stream = nullptr, *d_out = nullptr, *d_scratch = nullptr;
    uint64_t* d_boff = nullptr;
    snappy_hip_stream_desc* d_desc = nullptr;
    snappy_hip_range* d_range = nullptr;
    uint32_t* d_status = nullptr;
    if (snappy_status st = call.buffers({{&d_stream, in_len}, {&d_boff, (span.last + 1) * sizeof(uint64_t)}, {&d_desc, sizeof *d_desc},
                                         {&d_range, sizeof *d_range}, {&d_status, sizeof *d_status}, {&d_out, length},
                                         {&d_scratch, scratch_bytes}}))
        return st;
    const snappy_hip_stream_desc desc{d_stream, in_len, d_boff, nullptr, c.total, c.bs, c.hdr, (uint32_t)(span.last + 1)};
    const snappy_hip_range range{offset, length, d_out, 0, 0};
    if (snappy_status st = call.upload({{d_stream, buf + in_lo, in_len}, {d_boff, off.data(), (span.last + 1) * sizeof(uint64_t)},
                                        {d_desc, &desc, sizeof desc}, {d_range, &range, sizeof range}}))
        return st;
    if (snappy_status st = call.launch("range decode", [&] {
            return snappy_hip_decompress_ranges(d_desc, 1, d_range, 1, d_status, c.bs, d_scratch, scratch_bytes, nullptr);
        }))
        return st;
    uint32_t status = 0xffffffffu;
    if (snappy_status st = call.copy_out([&] {
            return call.download({{&status, d_status, sizeof status}, {output->buffer, d_out, length}});
        }))
        return st;
    if (snappy_status st = call.free_buffers()) return st;
    if (status != SNAPPY_HIP_BLOCK_OK) {
        fprintf(stderr, "snappy_hip: a block of the range [%lu, %lu) does not decode (status %u)\n", (unsigned long)offset,
                (unsigned long)(offset + length), status);
        return SNAPPY_INVALID_INPUT;
    }
    place(output, length);
    return SNAPPY_OK;
}

// A whole framed file through the wide decoder (snappy_decompress_wide_gpu): the header and the whole size chain on the host,
// the whole stream to the device, one snappy_hip_decompress_blocks_wide, the plaintext back.
snappy_status decompress_wide_gpu_body(struct host_buffer_context* input, struct host_buffer_context* output, uint32_t waves_per_block,
                                       struct program_runtime* runtime)
{
    if (!input || !output || !runtime || !input->buffer) return SNAPPY_INVALID_INPUT;
    PhasedCall call(runtime);
    if (waves_per_block != 0 && waves_per_block != 2 && waves_per_block != 4 && waves_per_block != 8 && waves_per_block != 16)
        return say(dropin_plan::refuse("waves_per_block %u is not 0, 2, 4, 8 or 16", waves_per_block));
    const uint8_t* const buf = input->buffer;
    const uint64_t in_total = input->length;
    const dropin_plan::Container c = dropin_plan::open_container(buf, in_total);
    const uint64_t nb = c.nb;
    std::vector<uint64_t> off;
    if (const dropin_plan::Verdict v = dropin_plan::walk_to(buf, in_total, c, nb, true, off)) return say(v);
    const uint64_t total = c.total;
    if (snappy_status st = claim_output(output, total)) return st;
    place(output, 0);
    if (total == 0) return call.done_on_host();
    if (snappy_status st = call.need_device()) return st;

    uint8_t *d_stream = nullptr, *d_out = nullptr;
    uint64_t* d_boff = nullptr;
    uint32_t *d_status = nullptr, *d_result = nullptr;
    if (snappy_status st = call.buffers({{&d_stream, in_total}, {&d_boff, nb * sizeof(uint64_t)}, {&d_status, nb * sizeof(uint32_t)},
                                         {&d_result, 4 * sizeof(uint32_t)}, {&d_out, total}}))
        return st;
    if (snappy_status st = call.upload({{d_stream, buf, in_total}, {d_boff, off.data(), nb * sizeof(uint64_t)}})) return st;
    if (snappy_status st = call.launch("wide decode", [&] {
            return snappy_hip_decompress_blocks_wide(d_stream, in_total, d_boff, total, c.bs, d_out, d_status, waves_per_block, d_result, nullptr);
        }))
        return st;
    std::vector<uint32_t> status(nb, 0xffffffffu);
    uint64_t bad = 0, first_bad = 0;
    if (snappy_status st = call.copy_out([&]() -> int {
            if (int rc = call.download({{status.data(), d_status, nb * sizeof(uint32_t)}})) return rc;
            for (uint64_t b = nb; b-- > 0;)
                if (status[b] != SNAPPY_HIP_BLOCK_OK) {
                    ++bad;
                    first_bad = b;
                }
            return bad ? 0 : call.download({{output->buffer, d_out, total}});
        }))
        return st;
    if (snappy_status st = call.free_buffers()) return st;
    if (bad) {
        fprintf(stderr, "snappy_hip: %lu of %lu blocks do not decode, the first is block %lu\n", (unsigned long)bad, (unsigned long)nb,
                (unsigned long)first_bad);
        return SNAPPY_INVALID_INPUT;
    }
    place(output, total);
    return SNAPPY_OK;
}

// One overwrite of a framed file (snappy_update_range_gpu): the header and the whole size chain on the host, the whole stream
// to the device, one write through snappy_hip_update_ranges, the new stream back.  `output` is left alone until it succeeds.
snappy_status update_range_gpu_body(struct host_buffer_context* input, struct host_buffer_context* patch, uint64_t offset,
                                    struct host_buffer_context* output, struct program_runtime* runtime)
{
    if (!input || !patch || !output || !runtime || !input->buffer || (patch->length && !patch->buffer)) return SNAPPY_INVALID_INPUT;
    PhasedCall call(runtime);
    const uint8_t* const buf = input->buffer;
    const uint64_t in_total = input->length, length = patch->length;
    const dropin_plan::Container c = dropin_plan::open_container(buf, in_total);
    dropin_plan::Span span;
    if (const dropin_plan::Verdict v = dropin_plan::resolve_span(c, offset, length, "write", &span)) return say(v);
    const uint64_t nb = c.nb;
    std::vector<uint64_t> off;
    if (const dropin_plan::Verdict v = dropin_plan::walk_to(buf, in_total, c, nb, true, off)) return say(v);
    if (snappy_status st = call.need_device()) return st;
    const uint32_t dirty_max = (uint32_t)span.blocks;
    const uint32_t bs_arg = c.total ? c.bs : 32768u;      // (an empty container's block size may be anything: nothing is sized by it)
    // a dirty block grows to a slot at most, a clean one keeps its size
    const uint64_t capacity = in_total + (uint64_t)dirty_max * snappy_hip_slot_stride(bs_arg) + 16;
    const uint64_t scratch_bytes = snappy_hip_update_scratch_bytes(bs_arg, (uint32_t)nb, 1, std::max(1u, dirty_max));

    uint8_t *d_stream = nullptr, *d_new = nullptr, *d_scratch = nullptr, *d_patch = nullptr;
    uint64_t *d_boff = nullptr, *d_noff = nullptr;      // d_noff: the new offsets, then the new length
    snappy_hip_stream_desc* d_desc = nullptr;
    snappy_hip_write* d_write = nullptr;
    uint32_t* d_words = nullptr;                        // [0] the write's status, [1..2] the result
    if (snappy_status st = call.buffers({{&d_stream, in_total}, {&d_boff, (nb + 1) * sizeof(uint64_t)}, {&d_noff, (nb + 2) * sizeof(uint64_t)},
                                         {&d_desc, sizeof *d_desc}, {&d_write, sizeof *d_write}, {&d_words, 4 * sizeof(uint32_t)},
                                         {&d_patch, length}, {&d_new, capacity}, {&d_scratch, scratch_bytes}}))
        return st;
    const snappy_hip_stream_desc desc{d_stream, in_total, d_boff, nullptr, c.total, bs_arg, c.hdr, (uint32_t)nb};
    const snappy_hip_write write{offset, length, d_patch, 0};
    if (snappy_status st = call.upload({{d_stream, buf, in_total}, {d_boff, off.data(), (nb + 1) * sizeof(uint64_t)}, {d_desc, &desc, sizeof desc},
                                        {d_write, &write, sizeof write}, {d_patch, patch->buffer, length}}))
        return st;
    if (snappy_status st = call.launch("update", [&] {
            return snappy_hip_update_ranges(d_desc, c.total, bs_arg, d_write, 1, d_words, d_new, capacity, d_noff, d_noff + nb + 1, d_words + 1,
                                            std::max(1u, dirty_max), d_scratch, scratch_bytes, nullptr);
        }))
        return st;
    uint32_t words[3] = {0xffffffffu, 0xffffffffu, 0};
    uint64_t new_len = 0;
    snappy_status verdict = SNAPPY_OK;
    if (snappy_status st = call.copy_out([&]() -> int {
            if (int rc = call.download({{words, d_words, sizeof words}, {&new_len, d_noff + nb + 1, sizeof new_len}})) return rc;
            if (words[0] != SNAPPY_HIP_BLOCK_OK || words[1] != SNAPPY_HIP_BLOCK_OK || new_len > capacity) {
                fprintf(stderr, "snappy_hip: the stream cannot be updated (write status %u, result %u)\n", words[0], words[1]);
                verdict = SNAPPY_INVALID_INPUT;
                return 0;
            }
            if ((verdict = claim_output(output, new_len))) return 0;
            return call.download({{output->buffer, d_new, new_len}});
        }))
        return st;
    if (verdict) return verdict;
    if (snappy_status st = call.free_buffers()) return st;
    place(output, new_len);
    return SNAPPY_OK;
}

// One resize of a framed file (snappy_resize_gpu): the header and the whole size chain on the host (in parallel shares where
// the stream is long enough, csrc/host_chain.hpp), the whole stream and the tail to the device, one segment through
// snappy_hip_resize, the new stream back.  `output` is left alone until it succeeds.
snappy_status resize_gpu_body(struct host_buffer_context* input, uint64_t keep_len, struct host_buffer_context* tail,
                              struct host_buffer_context* output, struct program_runtime* runtime)
{
    if (!input || !output || !runtime || !input->buffer || (tail && tail->length && !tail->buffer)) return SNAPPY_INVALID_INPUT;
    PhasedCall call(runtime);
    const uint8_t* const buf = input->buffer;
    const uint64_t in_total = input->length, length = tail ? tail->length : 0;
    const dropin_plan::Container c = dropin_plan::open_container(buf, in_total);
    if (!c.hdr) return say(c.bad);
    if (keep_len > c.total) return say(dropin_plan::refuse("keep length %lu lies beyond the %u uncompressed bytes", (unsigned long)keep_len, c.total));
    if (length > 0xffffffffull - keep_len)
        return say(dropin_plan::refuse("%lu + %lu bytes do not fit the format's 32-bit length", (unsigned long)keep_len, (unsigned long)length));
    if (!block_size_ok(c.bs)) return say(dropin_plan::bad_block_size(c.bs, " in the stream"));
    const uint64_t nb = c.nb;
    std::vector<uint64_t> off;
    const unsigned walk_threads = (unsigned)std::max(1, env_int("SNAPPY_HIP_HOST_WALK_THREADS",
                                                               (int)std::min(16u, std::max(1u, std::thread::hardware_concurrency()))));
    if (!host_chain::parallel_walk(buf, in_total, c.hdr, nb, c.bs, walk_threads, off))
        if (const dropin_plan::Verdict v = dropin_plan::walk_to(buf, in_total, c, nb, true, off)) return say(v);
    if (snappy_status st = call.need_device()) return st;
    const uint32_t keep = (uint32_t)keep_len, new_total = (uint32_t)(keep_len + length);
    const uint64_t new_nb = snappy_hip_num_blocks(new_total, c.bs), kept = keep / c.bs;
    // a kept block keeps its size, a compressed one grows to a slot at most
    const uint64_t capacity = 16 + (kept ? off[kept] : 0) + (new_nb - kept) * snappy_hip_slot_stride(c.bs);
    const uint64_t scratch_bytes = snappy_hip_resize_scratch_bytes(c.bs, (uint32_t)nb, new_total, keep, 1);

    uint8_t *d_stream = nullptr, *d_new = nullptr, *d_scratch = nullptr, *d_tail = nullptr;
    uint64_t *d_boff = nullptr, *d_noff = nullptr;      // d_noff: the new offsets, then the new length
    snappy_hip_stream_desc* d_desc = nullptr;
    snappy_hip_segment* d_segment = nullptr;
    uint32_t* d_words = nullptr;                        // [0] the segment's status, [1..2] the result
    if (snappy_status st = call.buffers({{&d_stream, in_total}, {&d_boff, (nb + 1) * sizeof(uint64_t)}, {&d_noff, (new_nb + 2) * sizeof(uint64_t)},
                                         {&d_desc, sizeof *d_desc}, {&d_segment, sizeof *d_segment}, {&d_words, 4 * sizeof(uint32_t)},
                                         {&d_tail, length}, {&d_new, capacity}, {&d_scratch, scratch_bytes}}))
        return st;
    const snappy_hip_stream_desc desc{d_stream, in_total, d_boff, nullptr, c.total, c.bs, c.hdr, (uint32_t)nb};
    const snappy_hip_segment segment{d_tail, length};
    if (snappy_status st = call.upload({{d_stream, buf, in_total}, {d_boff, off.data(), (nb + 1) * sizeof(uint64_t)}, {d_desc, &desc, sizeof desc},
                                        {d_segment, &segment, sizeof segment}, {d_tail, tail ? tail->buffer : nullptr, length}}))
        return st;
    if (snappy_status st = call.launch("resize", [&] {
            return snappy_hip_resize(d_desc, c.total, c.bs, keep, new_total, d_segment, 1, d_words, d_new, capacity, d_noff, d_noff + new_nb + 1,
                                     d_words + 1, d_scratch, scratch_bytes, nullptr);
        }))
        return st;
    uint32_t words[3] = {0xffffffffu, 0xffffffffu, 0};
    uint64_t new_len = 0;
    snappy_status verdict = SNAPPY_OK;
    if (snappy_status st = call.copy_out([&]() -> int {
            if (int rc = call.download({{words, d_words, sizeof words}, {&new_len, d_noff + new_nb + 1, sizeof new_len}})) return rc;
            if (words[0] != SNAPPY_HIP_BLOCK_OK || words[1] != SNAPPY_HIP_BLOCK_OK || new_len > capacity) {
                fprintf(stderr, "snappy_hip: the stream cannot be resized (segment status %u, result %u)\n", words[0], words[1]);
                verdict = SNAPPY_INVALID_INPUT;
                return 0;
            }
            if ((verdict = claim_output(output, new_len))) return 0;
            return call.download({{output->buffer, d_new, new_len}});
        }))
        return st;
    if (verdict) return verdict;
    if (snappy_status st = call.free_buffers()) return st;
    place(output, new_len);
    return SNAPPY_OK;
}

// The raw ("original") Snappy format, one buffer each way: one item through the batch calls of snappy_raw.hpp.
struct RawVerdict {            // what one item's call leaves on the device
    uint64_t out_len;
    uint32_t status;
    uint32_t result[4];        // (compress: two words; the split decode: four)
    uint32_t pad;
};

// compress = true: plaintext -> raw stream at `block_size` fragments; false: raw stream -> plaintext, by one wavefront, or --
// split_unit >= 0 -- by snappy_hip_raw_decompress_split_batch at that unit_len (0 = its default), limits sized from the file.
// tables (compress): through snappy_hip_raw_compress_batch_tables with a table workspace of the full grid.
snappy_status raw_gpu_body(bool compress, struct host_buffer_context* input, struct host_buffer_context* output, uint32_t block_size,
                           struct program_runtime* runtime, int64_t split_unit = -1, bool tables = false)
{
    if (!input || !output || !runtime || (!input->buffer && input->length)) return SNAPPY_INVALID_INPUT;
    PhasedCall call(runtime);
    const uint64_t in_len = input->length;
    uint64_t capacity = 0, scratch_bytes = 0, segments = 0, units = 0;
    uint32_t fragments = 0, unit_len = 0;
    if (compress) {
        if (!block_size_ok(block_size)) return say(dropin_plan::bad_block_size(block_size, ""));
        if (in_len >> 32) {
            fprintf(stderr, "snappy_hip: a raw Snappy stream holds less than 4 GiB\n");
            return SNAPPY_INVALID_INPUT;
        }
        fragments = (uint32_t)snappy_hip_num_blocks(in_len, block_size);
        capacity = snappy_hip_raw_compress_bound(in_len, block_size);
        scratch_bytes = snappy_hip_raw_compress_scratch_bytes(block_size, 1, fragments);
    } else {
        uint32_t length = 0;
        if (!get_varint32(input->buffer, in_len, &length)) return say(dropin_plan::unreadable_header());   // (the device reads it again, by Google's rule)
        if (in_len > SNAPPY_HIP_RAW_MAX_LEN || length > SNAPPY_HIP_RAW_MAX_LEN) {
            fprintf(stderr, "snappy_hip: raw streams of more than %llu bytes are not decoded\n", (unsigned long long)SNAPPY_HIP_RAW_MAX_LEN);
            return SNAPPY_INVALID_INPUT;
        }
        capacity = length;
        if (split_unit >= 0) {
            if (split_unit > 0xffffffffll || (split_unit && split_unit < 256)) {
                fprintf(stderr, "snappy_hip: the unit length of a split decode is 0 (the default) or at least 256\n");
                return SNAPPY_INVALID_INPUT;
            }
            unit_len = split_unit ? (uint32_t)split_unit : 65536u;
            segments = in_len / 16384u + 1;                                     // (the default segment_bytes)
            units = (uint64_t)length / unit_len + 1;
            scratch_bytes = snappy_hip_raw_decompress_split_scratch_bytes(1, unit_len, 0, segments, units);
        }
        if (snappy_status st = claim_output(output, capacity)) return st;      // decode knows its size now, compress after the launch
    }
    place(output, 0);
    if (snappy_status st = call.need_device()) return st;

    uint8_t *d_in = nullptr, *d_out = nullptr, *d_scratch = nullptr, *d_tables = nullptr;
    snappy_hip_raw_item* d_item = nullptr;
    RawVerdict* d_verdict = nullptr;
    const uint64_t tables_bytes = tables ? snappy_hip_compress_scratch_bytes() : 0;
    if (snappy_status st = call.buffers({{&d_in, in_len}, {&d_out, capacity}, {&d_item, sizeof *d_item}, {&d_verdict, sizeof *d_verdict},
                                         {&d_scratch, scratch_bytes}, {&d_tables, tables_bytes}}))
        return st;
    const snappy_hip_raw_item item{d_in, in_len, d_out, capacity};
    if (snappy_status st = call.upload({{d_in, input->buffer, in_len}, {d_item, &item, sizeof item}})) return st;
    if (snappy_status st = call.launch("raw batch", [&] {
            return tables ? snappy_hip_raw_compress_batch_tables(d_item, 1, block_size, fragments, &d_verdict->out_len, &d_verdict->status,
                                                                 d_verdict->result, d_scratch, scratch_bytes, d_tables, tables_bytes, nullptr)
                   : compress ? snappy_hip_raw_compress_batch(d_item, 1, block_size, fragments, &d_verdict->out_len, &d_verdict->status,
                                                              d_verdict->result, d_scratch, scratch_bytes, nullptr)
                   : split_unit >= 0
                       ? snappy_hip_raw_decompress_split_batch(d_item, 1, unit_len, 0, segments, units, &d_verdict->out_len, &d_verdict->status,
                                                               d_verdict->result, d_scratch, scratch_bytes, nullptr)
                       : snappy_hip_raw_decompress_batch(d_item, 1, &d_verdict->out_len, &d_verdict->status, nullptr);
        }))
        return st;
    RawVerdict v{};
    snappy_status verdict = SNAPPY_OK;
    if (snappy_status st = call.copy_out([&]() -> int {
            if (int rc = call.download({{&v, d_verdict, sizeof v}})) return rc;
            if (v.status != SNAPPY_HIP_BLOCK_OK || v.out_len > capacity) {
                fprintf(stderr, "snappy_hip: the raw stream cannot be %s (status %u)\n", compress ? "written" : "decoded", v.status);
                verdict = SNAPPY_INVALID_INPUT;
                return 0;
            }
            if (compress && (verdict = claim_output(output, v.out_len))) return 0;
            return call.download({{output->buffer, d_out, v.out_len}});
        }))
        return st;
    if (verdict) return verdict;
    if (snappy_status st = call.free_buffers()) return st;
    place(output, v.out_len);
    return SNAPPY_OK;
}

// The Snappy framing format (.sz), one buffer each way: one item through the batch calls of snappy_sz.hpp.
struct SzVerdict {             // what one item's call leaves on the device
    uint64_t out_len;
    uint32_t status;
    uint32_t bad_chunk;
    uint32_t result[4];        // (the split call writes four words)
};

// The chunk chain of a .sz file by the rules of snappy_hip_sz_decompress_batch, to size the call: the number of data chunks and
// the sum of their uncompressed lengths.  nullptr, or why the chain does not parse (the device would say the same).
inline const char* sz_host_walk(const uint8_t* s, uint64_t len, uint64_t* chunks, uint64_t* total)
{
    uint64_t at = 0;
    bool identified = false;
    *chunks = *total = 0;
    while (at < len) {
        if (at + 4 > len) return "a chunk header runs past the end of the file";
        const uint32_t type = s[at], L = s[at + 1] | (uint32_t)s[at + 2] << 8 | (uint32_t)s[at + 3] << 16;
        if (at + 4 + L > len) return "a chunk runs past the end of the file";
        if (type == 0xffu) {
            if (L != 6 || memcmp(s + at + 4, "sNaPpY", 6) != 0) return "a wrong stream identifier";
            identified = true;
        } else if (!identified) {
            return "the first chunk is not the stream identifier";
        } else if (type <= 1u) {
            if (L < 4) return "a data chunk without room for its checksum";
            uint32_t n = L - 4;
            if (type == 0 && !get_varint32(s + at + 8, L - 4, &n)) return "a compressed chunk without a readable length";
            if (n > 65536u) return "a chunk of more than 65536 bytes";
            *total += n;
            ++*chunks;
        } else if (type < 0x80u) {
            return "a reserved unskippable chunk";
        }
        at += 4ull + L;
    }
    return identified ? nullptr : "no stream identifier";
}

// compress = true: plaintext -> .sz at chunk_len; false: .sz -> plaintext, every CRC compared unless flags says not to.
// split: the decode goes through snappy_hip_sz_decompress_split_batch at its default segment with a limit sized from the file.
// tables (compress): through snappy_hip_sz_compress_batch_tables with a table workspace of the full grid.
snappy_status sz_gpu_body(bool compress, struct host_buffer_context* input, struct host_buffer_context* output, uint32_t chunk_len, uint32_t flags,
                          struct program_runtime* runtime, bool split = false, bool tables = false)
{
    if (!input || !output || !runtime || (!input->buffer && input->length)) return SNAPPY_INVALID_INPUT;
    PhasedCall call(runtime);
    const uint64_t in_len = input->length;
    uint64_t capacity = 0, scratch_bytes = 0, chunks = 0;
    const uint64_t segments = (in_len >> 20) + 1;                           // (the default segment_bytes)
    if (compress) {
        if (!block_size_ok(chunk_len)) return say(dropin_plan::bad_block_size(chunk_len, ""));
        if (in_len >> 32) {
            fprintf(stderr, "snappy_hip: one .sz item holds less than 4 GiB\n");
            return SNAPPY_INVALID_INPUT;
        }
        chunks = snappy_hip_num_blocks(in_len, chunk_len);
        capacity = snappy_hip_sz_compress_bound(in_len, chunk_len);
        scratch_bytes = snappy_hip_sz_compress_scratch_bytes(chunk_len, 1, (uint32_t)chunks);
    } else {
        if (flags & ~SNAPPY_HIP_SZ_NO_VERIFY) return SNAPPY_INVALID_INPUT;
        const char* why = in_len > SNAPPY_HIP_RAW_MAX_LEN ? "the file is longer than SNAPPY_HIP_RAW_MAX_LEN" : sz_host_walk(input->buffer, in_len, &chunks, &capacity);
        if (!why && capacity > SNAPPY_HIP_RAW_MAX_LEN) why = "the plaintext is longer than SNAPPY_HIP_RAW_MAX_LEN";
        if (why) {
            (void)call.done_on_host();
            fprintf(stderr, "snappy_hip: not a readable .sz stream: %s\n", why);
            return SNAPPY_INVALID_INPUT;
        }
        scratch_bytes = split ? snappy_hip_sz_decompress_split_scratch_bytes(1, (uint32_t)chunks, 0, segments)
                              : snappy_hip_sz_decompress_scratch_bytes(1, (uint32_t)chunks);
        if (snappy_status st = claim_output(output, capacity)) return st;
    }
    place(output, 0);
    if (snappy_status st = call.need_device()) return st;

    uint8_t *d_in = nullptr, *d_out = nullptr, *d_scratch = nullptr, *d_tables = nullptr;
    snappy_hip_raw_item* d_item = nullptr;
    SzVerdict* d_verdict = nullptr;
    const uint64_t tables_bytes = tables ? snappy_hip_compress_scratch_bytes() : 0;
    if (snappy_status st = call.buffers({{&d_in, in_len}, {&d_out, capacity}, {&d_item, sizeof *d_item}, {&d_verdict, sizeof *d_verdict},
                                         {&d_scratch, scratch_bytes}, {&d_tables, tables_bytes}}))
        return st;
    const snappy_hip_raw_item item{d_in, in_len, d_out, capacity};
    if (snappy_status st = call.upload({{d_in, input->buffer, in_len}, {d_item, &item, sizeof item}})) return st;
    if (snappy_status st = call.launch("sz batch", [&] {
            return tables   ? snappy_hip_sz_compress_batch_tables(d_item, 1, chunk_len, (uint32_t)chunks, &d_verdict->out_len, &d_verdict->status,
                                                                  d_verdict->result, d_scratch, scratch_bytes, d_tables, tables_bytes, nullptr)
                   : compress ? snappy_hip_sz_compress_batch(d_item, 1, chunk_len, (uint32_t)chunks, &d_verdict->out_len, &d_verdict->status,
                                                           d_verdict->result, d_scratch, scratch_bytes, nullptr)
                   : split  ? snappy_hip_sz_decompress_split_batch(d_item, 1, (uint32_t)chunks, 0, segments, flags, &d_verdict->out_len,
                                                                   &d_verdict->status, &d_verdict->bad_chunk, d_verdict->result, d_scratch,
                                                                   scratch_bytes, nullptr)
                            : snappy_hip_sz_decompress_batch(d_item, 1, (uint32_t)chunks, flags, &d_verdict->out_len, &d_verdict->status,
                                                             &d_verdict->bad_chunk, d_verdict->result, d_scratch, scratch_bytes, nullptr);
        }))
        return st;
    SzVerdict v{};
    snappy_status verdict = SNAPPY_OK;
    if (snappy_status st = call.copy_out([&]() -> int {
            if (int rc = call.download({{&v, d_verdict, sizeof v}})) return rc;
            if (v.status != SNAPPY_HIP_BLOCK_OK || v.out_len > capacity) {
                if (!compress && (v.status == SNAPPY_HIP_SZ_CRC_MISMATCH || v.status == SNAPPY_HIP_BLOCK_INVALID))
                    fprintf(stderr, "snappy_hip: data chunk %u of the .sz stream %s\n", v.bad_chunk,
                            v.status == SNAPPY_HIP_SZ_CRC_MISMATCH ? "fails its CRC-32C" : "does not decode");
                else
                    fprintf(stderr, "snappy_hip: the .sz stream cannot be %s (status %u)\n", compress ? "written" : "decoded", v.status);
                verdict = SNAPPY_INVALID_INPUT;
                return 0;
            }
            if (compress && (verdict = claim_output(output, v.out_len))) return 0;
            return call.download({{output->buffer, d_out, v.out_len}});
        }))
        return st;
    if (verdict) return verdict;
    if (snappy_status st = call.free_buffers()) return st;
    place(output, v.out_len);
    return SNAPPY_OK;
}

// One byte range of a .sz file's plaintext (snappy_decompress_sz_range_gpu): the chunk chain on the host only up to the last chunk
// the range touches (sz_host_walk's tests, chunk by chunk), only the touched chunks' bytes and their records -- rebased to the
// copied span -- to the device, one range through snappy_hip_sz_decompress_ranges, `length` bytes back.
snappy_status sz_range_gpu_body(struct host_buffer_context* input, struct host_buffer_context* output, uint64_t offset, uint64_t length,
                                uint32_t flags, struct program_runtime* runtime)
{
    if (!input || !output || !runtime || (!input->buffer && input->length)) return SNAPPY_INVALID_INPUT;
    if (flags & ~SNAPPY_HIP_SZ_NO_VERIFY) return SNAPPY_INVALID_INPUT;
    PhasedCall call(runtime);
    const uint8_t* const s = input->buffer;
    const uint64_t len = input->length, end = offset + length;
    const char* why = end < offset ? "the range overflows" : len > SNAPPY_HIP_RAW_MAX_LEN ? "the file is longer than SNAPPY_HIP_RAW_MAX_LEN" : nullptr;
    std::vector<snappy_hip_sz_chunk> recs;      // the touched chunks: dst_off + ulen > offset and dst_off < end (the device's first..last)
    uint64_t at = 0, total = 0, first_k = 0, k = 0;
    bool identified = false;
    while (!why && at < len && !(identified && total >= end)) {
        if (at + 4 > len) why = "a chunk header runs past the end of the file";
        if (why) break;
        const uint32_t type = s[at], L = s[at + 1] | (uint32_t)s[at + 2] << 8 | (uint32_t)s[at + 3] << 16;
        if (at + 4 + L > len) {
            why = "a chunk runs past the end of the file";
        } else if (type == 0xffu) {
            if (L != 6 || memcmp(s + at + 4, "sNaPpY", 6) != 0) why = "a wrong stream identifier";
            identified = true;
        } else if (!identified) {
            why = "the first chunk is not the stream identifier";
        } else if (type <= 1u) {
            uint32_t n = L - 4, hdr = 0;
            if (L < 4) why = "a data chunk without room for its checksum";
            else if (type == 0 && !(hdr = get_varint32(s + at + 8, L - 4, &n))) why = "a compressed chunk without a readable length";
            else if (n > 65536u) why = "a chunk of more than 65536 bytes";
            if (why) break;
            if (length && total < end && total + n > offset) {
                if (recs.empty()) first_k = k;
                recs.push_back(snappy_hip_sz_chunk{at, total, L | (hdr << 24) | (type == 0 ? 1u << 28 : 0u), n, 0, 0});
            }
            total += n;
            ++k;
        } else if (type < 0x80u) {
            why = "a reserved unskippable chunk";
        }
        at += 4ull + L;
    }
    if (!why && !identified) why = "no stream identifier";
    if (why) {
        (void)call.done_on_host();
        fprintf(stderr, "snappy_hip: not a readable .sz stream in front of the range's end: %s\n", why);
        return SNAPPY_INVALID_INPUT;
    }
    if (total < end) {
        (void)call.done_on_host();
        fprintf(stderr, "snappy_hip: the range [%lu, %lu) lies beyond the plaintext of %lu bytes\n", (unsigned long)offset, (unsigned long)end,
                (unsigned long)total);
        return SNAPPY_INVALID_INPUT;
    }
    if (snappy_status st = claim_output(output, length)) return st;
    place(output, 0);
    if (length == 0) return call.done_on_host();
    const uint64_t in_lo = recs.front().src_off, in_len = recs.back().src_off + 4 + (recs.back().info & 0xffffffu) - in_lo;
    for (snappy_hip_sz_chunk& r : recs) r.src_off -= in_lo;
    if (snappy_status st = call.need_device()) return st;
    const uint64_t cap = range_grid_cap();
    const uint64_t scratch_bytes = snappy_hip_sz_decompress_ranges_scratch_bytes(1) - cap * 65536u + std::min<uint64_t>(recs.size(), cap) * 65536u;

    uint8_t *d_in = nullptr, *d_out = nullptr, *d_scratch = nullptr;
    snappy_hip_sz_chunk* d_chunks = nullptr;
    snappy_hip_sz_desc* d_desc = nullptr;
    snappy_hip_range* d_range = nullptr;
    uint32_t* d_words = nullptr;                // [0] the range's status, [1] its bad chunk
    if (snappy_status st = call.buffers({{&d_in, in_len}, {&d_chunks, recs.size() * sizeof(snappy_hip_sz_chunk)}, {&d_desc, sizeof *d_desc},
                                         {&d_range, sizeof *d_range}, {&d_words, 2 * sizeof(uint32_t)}, {&d_out, length}, {&d_scratch, scratch_bytes}}))
        return st;
    const snappy_hip_sz_desc desc{d_in, in_len, d_chunks, recs.size(), total};
    const snappy_hip_range range{offset, length, d_out, 0, 0};
    if (snappy_status st = call.upload({{d_in, s + in_lo, in_len}, {d_chunks, recs.data(), recs.size() * sizeof(snappy_hip_sz_chunk)},
                                        {d_desc, &desc, sizeof desc}, {d_range, &range, sizeof range}}))
        return st;
    if (snappy_status st = call.launch("sz range decode", [&] {
            return snappy_hip_sz_decompress_ranges(d_desc, 1, d_range, 1, flags, d_words, d_words + 1, d_scratch, scratch_bytes, nullptr);
        }))
        return st;
    uint32_t words[2] = {0xffffffffu, 0xffffffffu};
    if (snappy_status st = call.copy_out([&]() -> int {
            if (int rc = call.download({{words, d_words, sizeof words}})) return rc;
            return words[0] == SNAPPY_HIP_BLOCK_OK ? call.download({{output->buffer, d_out, length}}) : 0;
        }))
        return st;
    if (snappy_status st = call.free_buffers()) return st;
    if (words[0] == SNAPPY_HIP_SZ_CRC_MISMATCH || words[0] == SNAPPY_HIP_BLOCK_INVALID) {
        fprintf(stderr, "snappy_hip: data chunk %lu of the .sz stream %s\n", (unsigned long)(first_k + words[1]),
                words[0] == SNAPPY_HIP_SZ_CRC_MISMATCH ? "fails its CRC-32C" : "does not decode");
        return SNAPPY_INVALID_INPUT;
    }
    if (words[0] != SNAPPY_HIP_BLOCK_OK) {
        fprintf(stderr, "snappy_hip: the range [%lu, %lu) of the .sz stream cannot be decoded (status %u)\n", (unsigned long)offset, (unsigned long)end,
                words[0]);
        return SNAPPY_INVALID_INPUT;
    }
    place(output, length);
    return SNAPPY_OK;
}

// Is a framed file intact (snappy_check_gpu)?  The header and the whole size chain on the host, the whole stream to the device,
// one snappy_hip_check_blocks, 16 bytes back.  A broken header or chain is decided here: nothing is sent to the device.
snappy_status check_gpu_body(struct host_buffer_context* input, snappy_hip_check_report* report, struct program_runtime* runtime)
{
    if (!input || !runtime || (!input->buffer && input->length)) return SNAPPY_INVALID_INPUT;
    PhasedCall call(runtime);
    snappy_hip_check_report none{};
    snappy_hip_check_report& rep = report ? *report : none;
    rep = snappy_hip_check_report{0, 0, ~0ull, ~0ull};
    const uint8_t* const buf = input->buffer;
    const uint64_t in_total = input->length;
    const dropin_plan::Container c = dropin_plan::open_container(buf, in_total);
    if (c.bad) {
        rep = snappy_hip_check_report{0, 1, 0, 0};
        (void)call.done_on_host();
        return say(c.bad);
    }
    const uint64_t nb = c.nb;
    rep.blocks = nb;
    std::vector<uint64_t> off;
    const unsigned walk_threads = (unsigned)std::max(1, env_int("SNAPPY_HIP_HOST_WALK_THREADS",
                                                               (int)std::min(16u, std::max(1u, std::thread::hardware_concurrency()))));
    if (!host_chain::parallel_walk(buf, in_total, c.hdr, nb, c.bs, walk_threads, off)) {
        // the serial walk, which also names the link that fails (every block needs its four size bytes: checked before
        // anything is sized by the header's count)
        const uint64_t fit = std::min<uint64_t>(nb, (in_total - c.hdr) / 4);
        off.assign(fit + 1, 0);
        const dropin_plan::Walk w = dropin_plan::walk_chain(buf, in_total, 0, off.data(), {0, c.hdr}, fit);
        const bool stopped = w.stop != dropin_plan::kDone || fit < nb;
        if (stopped || w.at != in_total) {
            rep.bad_blocks = 1;
            rep.first_bad_block = stopped ? w.block : (nb ? nb - 1 : 0);
            rep.first_bad_offset = !stopped ? (nb ? off[nb - 1] : c.hdr) : (w.stop == dropin_plan::kLeaves ? off[w.block] : w.at);
            (void)call.done_on_host();
            if (stopped) return say(dropin_plan::refuse("truncated stream (block %lu of %lu)", (unsigned long)rep.first_bad_block, (unsigned long)nb));
            return say(dropin_plan::refuse("%lu bytes behind the last block", (unsigned long)(in_total - w.at)));
        }
    }
    if (nb == 0) return call.done_on_host();
    if (snappy_status st = call.need_device()) return st;
    const uint64_t scratch_bytes = snappy_hip_check_scratch_bytes(1);

    uint8_t *d_stream = nullptr, *d_scratch = nullptr;
    uint64_t* d_boff = nullptr;
    snappy_hip_stream_desc* d_desc = nullptr;
    uint32_t* d_result = nullptr;
    if (snappy_status st = call.buffers({{&d_stream, in_total}, {&d_boff, nb * sizeof(uint64_t)}, {&d_desc, sizeof *d_desc},
                                         {&d_result, 4 * sizeof(uint32_t)}, {&d_scratch, scratch_bytes}}))
        return st;
    const snappy_hip_stream_desc desc{d_stream, in_total, d_boff, nullptr, c.total, c.bs, c.hdr, (uint32_t)nb};
    if (snappy_status st = call.upload({{d_stream, buf, in_total}, {d_boff, off.data(), nb * sizeof(uint64_t)}, {d_desc, &desc, sizeof desc}}))
        return st;
    if (snappy_status st = call.launch("check", [&] { return snappy_hip_check_blocks(d_desc, 1, nullptr, d_result, d_scratch, scratch_bytes, nullptr); }))
        return st;
    uint32_t words[4] = {0xffffffffu, 0, 0, 0};
    if (snappy_status st = call.copy_out([&] { return call.download({{words, d_result, sizeof words}}); })) return st;
    if (snappy_status st = call.free_buffers()) return st;
    if (words[0] == SNAPPY_HIP_BLOCK_OK) return SNAPPY_OK;
    if (words[0] == SNAPPY_HIP_BLOCK_INVALID && words[2] < nb) {
        rep.bad_blocks = words[1];
        rep.first_bad_block = words[2];
        rep.first_bad_offset = off[words[2]];
        fprintf(stderr, "snappy_hip: %u of %lu blocks do not decode, the first is block %u at offset %lu\n", words[1], (unsigned long)nb, words[2],
                (unsigned long)off[words[2]]);
    } else {
        rep.bad_blocks = nb;
        rep.first_bad_block = 0;
        rep.first_bad_offset = off[0];
        fprintf(stderr, "snappy_hip: the check did not run (result %u)\n", words[0]);
    }
    return SNAPPY_INVALID_INPUT;
}

// Is a raw Snappy file intact (snappy_check_raw_gpu)?  One item through snappy_hip_raw_check_batch, or -- split, snappy_check_raw_split_gpu --
// through snappy_hip_raw_check_split_batch at its default segment with a limit sized from the file.
snappy_status check_raw_gpu_body(struct host_buffer_context* input, uint64_t* uncompressed_len, struct program_runtime* runtime, bool split = false)
{
    if (!input || !runtime || (!input->buffer && input->length)) return SNAPPY_INVALID_INPUT;
    PhasedCall call(runtime);
    if (uncompressed_len) *uncompressed_len = 0;
    const uint64_t in_len = input->length;
    uint32_t length = 0;
    if (!get_varint32(input->buffer, in_len, &length)) {
        (void)call.done_on_host();
        return say(dropin_plan::unreadable_header());                // (the device reads it again, by Google's rule)
    }
    if (in_len > SNAPPY_HIP_RAW_MAX_LEN || length > SNAPPY_HIP_RAW_MAX_LEN) {
        (void)call.done_on_host();
        fprintf(stderr, "snappy_hip: raw streams of more than %llu bytes are not checked\n", (unsigned long long)SNAPPY_HIP_RAW_MAX_LEN);
        return SNAPPY_INVALID_INPUT;
    }
    if (snappy_status st = call.need_device()) return st;
    const uint64_t segments = in_len / 16384u + 1;                          // (the default segment_bytes)
    const uint64_t scratch_bytes = split ? snappy_hip_raw_check_split_scratch_bytes(1, 0, segments) : 0;
    uint8_t *d_in = nullptr, *d_scratch = nullptr;
    snappy_hip_raw_item* d_item = nullptr;
    RawVerdict* d_verdict = nullptr;
    if (snappy_status st = call.buffers({{&d_in, in_len}, {&d_item, sizeof *d_item}, {&d_verdict, sizeof *d_verdict}, {&d_scratch, scratch_bytes}}))
        return st;
    const snappy_hip_raw_item item{d_in, in_len, nullptr, 0};
    if (snappy_status st = call.upload({{d_in, input->buffer, in_len}, {d_item, &item, sizeof item}})) return st;
    if (snappy_status st = call.launch("raw check", [&] {
            return split ? snappy_hip_raw_check_split_batch(d_item, 1, 0, segments, &d_verdict->out_len, &d_verdict->status, d_verdict->result,
                                                            d_scratch, scratch_bytes, nullptr)
                         : snappy_hip_raw_check_batch(d_item, 1, &d_verdict->out_len, &d_verdict->status, nullptr);
        }))
        return st;
    RawVerdict v{};
    v.status = 0xffffffffu;
    if (snappy_status st = call.copy_out([&] { return call.download({{&v, d_verdict, sizeof v}}); })) return st;
    if (snappy_status st = call.free_buffers()) return st;
    if (v.status != SNAPPY_HIP_BLOCK_OK) {
        fprintf(stderr, "snappy_hip: the raw stream does not decode (status %u)\n", v.status);
        return SNAPPY_INVALID_INPUT;
    }
    if (uncompressed_len) *uncompressed_len = v.out_len;
    return SNAPPY_OK;
}

// The exported pair: one call at a time per process (the cached pipeline streams and their page-locked scratch are per
// process; the reference's entry points are single-threaded and synchronous anyway, snappy_compress.c:618), the caller's
// current HIP device restored on every return path, and no C++ exception crosses the C boundary.
template <class Body>
snappy_status entry_guard(Body body)
{
    try {
        std::lock_guard<std::mutex> one_at_a_time(*pipeline_mutex());
        CallerDevice keep;
        return body();
    } catch (const std::bad_alloc&) {
        fprintf(stderr, "snappy_hip: out of host memory\n");
        return SNAPPY_BUFFER_TOO_SMALL;
    } catch (const std::exception& e) {
        fprintf(stderr, "snappy_hip: %s\n", e.what());
        return SNAPPY_INVALID_INPUT;
    } catch (...) {
        return SNAPPY_INVALID_INPUT;
    }
}

}  // namespace

extern "C" {

snappy_status snappy_compress_gpu(struct host_buffer_context* input, struct host_buffer_context* output, uint32_t block_size,
                                  struct program_runtime* runtime)
{
    return entry_guard([&] { return compress_gpu_body(input, output, block_size, runtime); });
}

snappy_status snappy_decompress_gpu(struct host_buffer_context* input, struct host_buffer_context* output,
                                    struct program_runtime* runtime)
{
    return entry_guard([&] { return decompress_gpu_body(input, output, runtime); });
}

snappy_status snappy_decompress_range_gpu(struct host_buffer_context* input, struct host_buffer_context* output, uint64_t offset,
                                          uint64_t length, struct program_runtime* runtime)
{
    return entry_guard([&] { return decompress_range_gpu_body(input, output, offset, length, runtime); });
}

snappy_status snappy_decompress_wide_gpu(struct host_buffer_context* input, struct host_buffer_context* output, uint32_t waves_per_block,
                                         struct program_runtime* runtime)
{
    return entry_guard([&] { return decompress_wide_gpu_body(input, output, waves_per_block, runtime); });
}

snappy_status snappy_update_range_gpu(struct host_buffer_context* input, struct host_buffer_context* patch, uint64_t offset,
                                      struct host_buffer_context* output, struct program_runtime* runtime)
{
    return entry_guard([&] { return update_range_gpu_body(input, patch, offset, output, runtime); });
}

snappy_status snappy_resize_gpu(struct host_buffer_context* input, uint64_t keep_len, struct host_buffer_context* tail,
                                struct host_buffer_context* output, struct program_runtime* runtime)
{
    return entry_guard([&] { return resize_gpu_body(input, keep_len, tail, output, runtime); });
}

snappy_status snappy_compress_raw_gpu(struct host_buffer_context* input, struct host_buffer_context* output, uint32_t block_size,
                                      struct program_runtime* runtime)
{
    return entry_guard([&] { return raw_gpu_body(true, input, output, block_size, runtime); });
}

snappy_status snappy_compress_raw_tables_gpu(struct host_buffer_context* input, struct host_buffer_context* output, uint32_t block_size,
                                             struct program_runtime* runtime)
{
    return entry_guard([&] { return raw_gpu_body(true, input, output, block_size, runtime, -1, true); });
}

snappy_status snappy_decompress_raw_gpu(struct host_buffer_context* input, struct host_buffer_context* output, struct program_runtime* runtime)
{
    return entry_guard([&] { return raw_gpu_body(false, input, output, 0, runtime); });
}

snappy_status snappy_decompress_raw_split_gpu(struct host_buffer_context* input, struct host_buffer_context* output, uint32_t unit_len,
                                              struct program_runtime* runtime)
{
    return entry_guard([&] { return raw_gpu_body(false, input, output, 0, runtime, (int64_t)unit_len); });
}

snappy_status snappy_compress_sz_gpu(struct host_buffer_context* input, struct host_buffer_context* output, uint32_t chunk_len,
                                     struct program_runtime* runtime)
{
    return entry_guard([&] { return sz_gpu_body(true, input, output, chunk_len, 0, runtime); });
}

snappy_status snappy_compress_sz_tables_gpu(struct host_buffer_context* input, struct host_buffer_context* output, uint32_t chunk_len,
                                            struct program_runtime* runtime)
{
    return entry_guard([&] { return sz_gpu_body(true, input, output, chunk_len, 0, runtime, false, true); });
}

snappy_status snappy_decompress_sz_gpu(struct host_buffer_context* input, struct host_buffer_context* output, uint32_t flags,
                                       struct program_runtime* runtime)
{
    return entry_guard([&] { return sz_gpu_body(false, input, output, 0, flags, runtime); });
}

snappy_status snappy_decompress_sz_split_gpu(struct host_buffer_context* input, struct host_buffer_context* output, uint32_t flags,
                                             struct program_runtime* runtime)
{
    return entry_guard([&] { return sz_gpu_body(false, input, output, 0, flags, runtime, true); });
}

snappy_status snappy_decompress_sz_range_gpu(struct host_buffer_context* input, struct host_buffer_context* output, uint64_t offset,
                                             uint64_t length, uint32_t flags, struct program_runtime* runtime)
{
    return entry_guard([&] { return sz_range_gpu_body(input, output, offset, length, flags, runtime); });
}

snappy_status snappy_check_gpu(struct host_buffer_context* input, snappy_hip_check_report* report, struct program_runtime* runtime)
{
    return entry_guard([&] { return check_gpu_body(input, report, runtime); });
}

snappy_status snappy_check_raw_gpu(struct host_buffer_context* input, uint64_t* uncompressed_len, struct program_runtime* runtime)
{
    return entry_guard([&] { return check_raw_gpu_body(input, uncompressed_len, runtime); });
}

snappy_status snappy_check_raw_split_gpu(struct host_buffer_context* input, uint64_t* uncompressed_len, struct program_runtime* runtime)
{
    return entry_guard([&] { return check_raw_gpu_body(input, uncompressed_len, runtime, true); });
}

}  // extern "C"
