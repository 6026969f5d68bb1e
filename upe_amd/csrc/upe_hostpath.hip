// upe_hostpath.hip — the entry points that take batches in host memory (include/upe_gpu.h):
// the host round trip (upe_gpu_process_host / _emit: chunks through a ring of device slots, the
// copies overlapped with the kernels), the zero-copy path over pinned, mapped host memory
// (upe_gpu_process_mapped / _emit) and the pinned-memory helpers.  Every batch goes through
// process_impl (upe_gpu.hip) as a Path::Host request; no kernel is defined here.
#include <pthread.h>
#include <sched.h>

#include <algorithm>
#include <atomic>
#include <condition_variable>
#include <functional>
#include <mutex>
#include <thread>
#include <vector>

#include "upe_ctx.h"

using namespace upe;

// A small pool of host threads that run one job over slices: job(slice, slices), the caller
// being slice 0 (upe_gpu_process_host_emit applies the returned records to the caller's frames
// with it while later chunks are on the link).  Threads are pinned to the GPU's NUMA-local CPUs.
struct UPE_INTERNAL ApplyPool {
    std::vector<std::thread> th;
    std::mutex mu;
    std::condition_variable go, done;
    std::function<void(unsigned, unsigned)> job;
    uint64_t gen = 0;
    unsigned left = 0;
    bool stop = false;

    ApplyPool(unsigned n, const std::vector<int>& cpus) {
        for (unsigned t = 0; t < n; ++t)
            th.emplace_back([this, t, n, cpus] {
                if (!cpus.empty()) {   // after the caller's CPU (local slot 0)
                    cpu_set_t one;
                    CPU_ZERO(&one);
                    CPU_SET(cpus[(1 + t) % cpus.size()], &one);
                    (void)pthread_setaffinity_np(pthread_self(), sizeof one, &one);
                }
                uint64_t seen = 0;
                for (;;) {
                    std::function<void(unsigned, unsigned)> f;
                    {
                        std::unique_lock<std::mutex> lk(mu);
                        go.wait(lk, [&] { return stop || gen != seen; });
                        if (stop) return;
                        seen = gen;
                        f = job;
                    }
                    f(t + 1, n + 1);
                    std::lock_guard<std::mutex> lk(mu);
                    if (--left == 0) done.notify_one();
                }
            });
    }
    ~ApplyPool() {
        {
            std::lock_guard<std::mutex> lk(mu);
            stop = true;
        }
        go.notify_all();
        for (auto& t : th) t.join();
    }
    void run(const std::function<void(unsigned, unsigned)>& f) {
        {
            std::lock_guard<std::mutex> lk(mu);
            job = f;
            left = (unsigned)th.size();
            ++gen;
        }
        go.notify_all();
        f(0, (unsigned)th.size() + 1);
        std::unique_lock<std::mutex> lk(mu);
        done.wait(lk, [&] { return left == 0; });
    }
};

// (here, where the pool's type is complete)
upe_gpu_ctx::HostPath::HostPath() = default;
upe_gpu_ctx::HostPath::~HostPath() = default;

namespace {
// The host round trip (upe_gpu_process_host / _emit): chunks of the caller's host batch through
// a ring of device slots, H2D on one copy stream, classify on the context's stream, D2H on a
// second copy stream.  In place: the rewritten span [lo, wb) of each chunk comes back.  Emit:
// the verdicts and the 16-byte records come back (20 B per packet instead of the span: the
// link's two directions share its bandwidth, so fewer bytes back let more go in), and when
// apply_threads >= 0 the records are applied to the caller's frames on the host two chunks
// behind, by the calling thread and `apply_threads` pool threads, while later chunks move.
int host_roundtrip(upe_gpu_ctx_t* c, uint8_t* h_frames, size_t frames_bytes,
                   const uint64_t* h_desc, uint32_t* h_verdict, upe_hdr_rec_t* h_hdr, size_t n,
                   size_t chunk, bool emit, int apply_threads) {
    if (!c) return fail("null context");
    if (n && (!h_frames || !h_desc || !h_verdict || (emit && !h_hdr))) return fail("null host buffer");
    DEV_SCOPE(c->device);
    // default chunks (round-3 sweep, config B 1M): in place 256k (479 Mpps; 128k 406, 64k 359),
    // emit 128k (559 Mpps; 256k 534, 64k 529)
    if (chunk == 0) chunk = emit ? (size_t)1 << 17 : (size_t)1 << 18;
    // emit: whole 64-packet groups per chunk, so that each chunk's compacted records (relative to
    // its first packet) land where the batch's own layout puts them
    if (emit) chunk = std::max<size_t>(64, chunk & ~(size_t)63);
    if (!c->host.s_in) {
        HIP_TRY(hipStreamCreateWithFlags(&c->host.s_in, hipStreamNonBlocking));
        HIP_TRY(hipStreamCreateWithFlags(&c->host.s_out, hipStreamNonBlocking));
        for (auto& sl : c->host.slots) {
            HIP_TRY(hipEventCreateWithFlags(&sl.in_done, hipEventDisableTiming));
            HIP_TRY(hipEventCreateWithFlags(&sl.k_done, hipEventDisableTiming));
            HIP_TRY(hipEventCreateWithFlags(&sl.out_done, hipEventDisableTiming));
        }
    }
    if (n == 0) {
        if (upe_gpu_process(c, nullptr, nullptr, nullptr, 0, nullptr) != 0) return -1;
        HIP_TRY(hipStreamSynchronize(c->stream));
        return 0;
    }
    const bool apply = emit && apply_threads >= 0;
    if (apply && apply_threads > 0 &&
        (!c->host.pool || c->host.pool->th.size() != (size_t)apply_threads)) {
        std::vector<int> cpus(CPU_SETSIZE);
        const int k = upe_gpu_local_cpus(c->device, cpus.data(), cpus.size(), nullptr);
        cpus.resize(k > 0 ? (size_t)k : 0);
        c->host.pool.reset();
        c->host.pool.reset(new ApplyPool((unsigned)apply_threads, cpus));
    }
    // Whatever happens below, no copy into the caller's buffers is left in flight on return.
    struct Drain {
        upe_gpu_ctx* c;
        ~Drain() {
            (void)hipStreamSynchronize(c->host.s_in);
            (void)hipStreamSynchronize(c->stream);
            (void)hipStreamSynchronize(c->host.s_out);
            for (auto& sl : c->host.slots) sl.busy = false;
        }
    } drain{c};
    const size_t nslots = c->host.nslots;
    // copies back on their own stream: both link directions at once (issuing them on the copy-in
    // stream after the next chunk's copy-in measured slower: B 332-344 vs 480 Mpps in place)
    hipStream_t s_back = c->host.s_out;
    const size_t lag = 2;   // emit: chunk k - lag is applied while chunk k is issued
    struct Done {
        size_t s, e, slot;
        uint64_t lo;
    };
    std::vector<Done> pending;
    // apply chunk d's records (and copy back its answered ARP requests, rewritten in place in
    // the device slot, which the reference transmits from b->data, src/worker.c:40-52)
    auto finish = [&](const Done& d) -> int {
        auto& sl = c->host.slots[d.slot];
        HIP_TRY(hipEventSynchronize(sl.out_done));
        std::atomic<bool> replies{false};
        auto job = [&](unsigned t, unsigned T) {
            const size_t m = d.e - d.s, a0 = d.s + m * t / T, a1 = d.s + m * (t + 1) / T;
            bool r = false;
            // the compacted record of the range's first forwarded packet
            size_t rec = a0 & ~(size_t)63;
            for (size_t j = rec; j < a0; ++j) rec += UPE_VERDICT_CODE(h_verdict[j]) == UPE_V_FWD;
            for (size_t i = a0; i < a1; ++i) {
                r |= (h_verdict[i] & UPE_VF_ARP_REPLY) != 0;
                if ((i & 63u) == 0) rec = i;
                if (UPE_VERDICT_CODE(h_verdict[i]) == UPE_V_FWD) {
                    if (apply) upe_hdr_apply(h_frames + (h_desc[i] >> 16), &h_hdr[rec]);
                    ++rec;
                }
            }
            if (r) replies.store(true, std::memory_order_relaxed);
        };
        if (c->host.pool && apply && apply_threads > 0) c->host.pool->run(job);
        else job(0, 1);
        if (replies.load())
            for (size_t i = d.s; i < d.e; ++i)
                if (h_verdict[i] & UPE_VF_ARP_REPLY) {
                    const uint64_t off = h_desc[i] >> 16, len = h_desc[i] & 0xFFFFu;
                    HIP_TRY(hipMemcpy(h_frames + off, sl.frames + (off - d.lo),
                                      len < UPE_REWRITE_EXTENT ? len : UPE_REWRITE_EXTENT,
                                      hipMemcpyDeviceToHost));
                }
        return 0;
    };
    // a chunk's copy-back (verdicts + records, or verdicts + the rewritten span), once its kernel
    // is queued
    auto issue_back = [&](size_t s, size_t e, size_t slot, uint64_t lo, uint64_t wb) -> int {
        auto& sb = c->host.slots[slot];
        const size_t m = e - s;
        HIP_TRY(hipStreamWaitEvent(s_back, sb.k_done, 0));
        HIP_TRY(hipMemcpyAsync(h_verdict + s, sb.verdict, m * sizeof(uint32_t),
                               hipMemcpyDeviceToHost, s_back));
        if (emit)
            HIP_TRY(hipMemcpyAsync(h_hdr + s, sb.hdr, m * sizeof(upe_hdr_rec_t),
                                   hipMemcpyDeviceToHost, s_back));
        else
            HIP_TRY(hipMemcpyAsync(h_frames + lo, sb.frames, (size_t)(wb - lo),
                                   hipMemcpyDeviceToHost, s_back));
        HIP_TRY(hipEventRecord(sb.out_done, s_back));
        sb.busy = true;
        sb.lo = lo;
        sb.wb = wb;
        return 0;
    };
    size_t k = 0;
    for (size_t s = 0; s < n; s += chunk, ++k) {
        const size_t e = n - s < chunk ? n : s + chunk, m = e - s;
        // The chunk's byte ranges: [lo, hi) holds every frame's window (the kernel reads up to
        // UPE_FRAME_TAIL bytes from a frame start), [lo, wb) every byte the kernel may rewrite.
        // The scan of chunk k+1 overlaps the copies and kernel of chunk k.
        uint64_t lo = ~0ull, hi = 0, wb = 0;
        for (size_t i = s; i < e; ++i) {
            const uint64_t off = h_desc[i] >> 16, len = h_desc[i] & 0xFFFFu;
            if (off & 15u) return fail("frame offsets must be multiples of 16 (include/upe_gpu.h)");
            lo = off < lo ? off : lo;
            hi = off + UPE_FRAME_TAIL > hi ? off + UPE_FRAME_TAIL : hi;
            const uint64_t w = off + (len < UPE_REWRITE_EXTENT ? len : UPE_REWRITE_EXTENT);
            wb = w > wb ? w : wb;
        }
        if (hi > frames_bytes)
            return fail("a frame window runs past frames_bytes (UPE_FRAME_TAIL bytes must follow "
                        "every frame start)");
        const size_t si = k % nslots;
        auto& sl = c->host.slots[si];
        if (emit && pending.size() >= lag) {   // the oldest finished before its slot is reused
            if (finish(pending.front()) != 0) return -1;
            pending.erase(pending.begin());
        }
        if (sl.busy) HIP_TRY(hipEventSynchronize(sl.out_done));   // the slot's last D2H is done
        sl.busy = false;
        const size_t span = (size_t)(hi - lo);
        if (sl.frames.reserve(span, span + span / 4) != 0) return -1;
        // (verdict, made after desc, holds the slot's packet capacity)
        if (m > sl.verdict.cap || (emit && !sl.hdr)) {
            const size_t cap = std::max(m, sl.verdict.cap);
            sl.desc.reset();
            sl.verdict.reset();
            sl.hdr.reset();
            if (sl.desc.reserve(cap, cap) != 0 || sl.verdict.reserve(cap, cap) != 0 ||
                (emit && sl.hdr.reserve(cap, cap) != 0))
                return -1;
        }
        // In place: a chunk whose bytes interleave with an earlier chunk's (descriptors in any
        // order, e.g. pool addresses) must read them only after that chunk's copy-back has
        // landed: its own copy-back rewrites its whole span, and would otherwise put back the
        // earlier chunk's frames as they were before they were processed.  (Emit mode copies
        // no frame bytes back.)
        if (!emit)
            for (auto& other : c->host.slots)
                if (&other != &sl && other.busy && other.lo < hi && lo < other.wb)
                    HIP_TRY(hipStreamWaitEvent(c->host.s_in, other.out_done, 0));
        HIP_TRY(hipMemcpyAsync(sl.frames, h_frames + lo, span, hipMemcpyHostToDevice, c->host.s_in));
        HIP_TRY(hipMemcpyAsync(sl.desc, h_desc + s, m * sizeof(uint64_t), hipMemcpyHostToDevice,
                               c->host.s_in));
        HIP_TRY(hipEventRecord(sl.in_done, c->host.s_in));
        HIP_TRY(hipStreamWaitEvent(c->stream, sl.in_done, 0));
        // the descriptors keep their offsets relative to h_frames: hand the kernel a base that
        // maps offset lo onto the slot (lo is a multiple of 16, so the base stays aligned)
        uint8_t* base = reinterpret_cast<uint8_t*>(reinterpret_cast<uintptr_t>(sl.frames.p) - lo);
        // (the host-path kernel instantiation: profiles keep these launches apart)
        ProcessReq q{base, sl.desc, sl.verdict, m, nullptr};
        q.hdr = emit ? sl.hdr.p : nullptr;
        q.host = true;
        if (process_impl(c, q) != 0) return -1;
        HIP_TRY(hipEventRecord(sl.k_done, c->stream));
        if (issue_back(s, e, si, lo, wb) != 0) return -1;
        if (emit) pending.push_back(Done{s, e, si, lo});
    }
    for (const Done& d : pending)
        if (finish(d) != 0) return -1;
    HIP_TRY(hipStreamSynchronize(s_back));
    return 0;
}
}  // namespace

extern "C" {

int upe_gpu_process_host(upe_gpu_ctx_t* c, uint8_t* h_frames, size_t frames_bytes,
                         const uint64_t* h_desc, uint32_t* h_verdict, size_t n, size_t chunk) {
    return host_roundtrip(c, h_frames, frames_bytes, h_desc, h_verdict, nullptr, n, chunk, false,
                          -1);
}

int upe_gpu_process_host_emit(upe_gpu_ctx_t* c, uint8_t* h_frames, size_t frames_bytes,
                              const uint64_t* h_desc, uint32_t* h_verdict, upe_hdr_rec_t* h_hdr,
                              size_t n, size_t chunk, int apply_threads) {
    if (apply_threads > 64) return fail("apply_threads must be at most 64");
    return host_roundtrip(c, h_frames, frames_bytes, h_desc, h_verdict, h_hdr, n, chunk, true,
                          apply_threads);
}

void* upe_gpu_host_alloc(size_t bytes) {
    void* p = nullptr;
    if (hipHostMalloc(&p, bytes ? bytes : 1, hipHostMallocDefault) != hipSuccess) {
        fail("hipHostMalloc failed");
        return nullptr;
    }
    return p;
}

int upe_gpu_host_free(void* p) {
    if (p) HIP_TRY(hipHostFree(p));
    return 0;
}

int upe_gpu_host_register(void* p, size_t bytes) {
    if (!p || !bytes) return fail("null or empty host buffer");
    HIP_TRY(hipHostRegister(p, bytes, hipHostRegisterMapped | hipHostRegisterPortable));
    return 0;
}

int upe_gpu_host_unregister(void* p) {
    if (!p) return fail("null host buffer");
    HIP_TRY(hipHostUnregister(p));
    return 0;
}

int upe_gpu_process_mapped(upe_gpu_ctx_t* c, uint8_t* h_frames, const uint64_t* h_desc,
                           uint32_t* h_verdict, size_t n, void* stream) {
    if (!c) return fail("null context");
    DEV_SCOPE(c->device);
    if (n == 0) return upe_gpu_process(c, nullptr, nullptr, nullptr, 0, stream);
    if (!h_frames || !h_desc || !h_verdict) return fail("null host buffer");
    uint8_t* f = mapped(h_frames, "h_frames");
    const uint64_t* d = f ? mapped(h_desc, "h_desc") : nullptr;
    uint32_t* v = d ? mapped(h_verdict, "h_verdict") : nullptr;
    if (!v) return -1;
    ProcessReq q{f, d, v, n, stream};
    q.host = true;
    return process_impl(c, q);
}

int upe_gpu_process_mapped_emit(upe_gpu_ctx_t* c, uint8_t* h_frames, const uint64_t* h_desc,
                                uint32_t* h_verdict, upe_hdr_rec_t* h_hdr, size_t n,
                                void* stream) {
    if (!c) return fail("null context");
    DEV_SCOPE(c->device);
    if (n == 0) return upe_gpu_process(c, nullptr, nullptr, nullptr, 0, stream);
    if (!h_frames || !h_desc || !h_verdict || !h_hdr) return fail("null host buffer");
    uint8_t* f = mapped(h_frames, "h_frames");
    const uint64_t* d = f ? mapped(h_desc, "h_desc") : nullptr;
    uint32_t* v = d ? mapped(h_verdict, "h_verdict") : nullptr;
    upe_hdr_rec_t* h = v ? mapped(h_hdr, "h_hdr") : nullptr;
    if (!h) return -1;
    ProcessReq q{f, d, v, n, stream};
    q.hdr = h;
    q.host = true;
    return process_impl(c, q);
}

}  // extern "C"
