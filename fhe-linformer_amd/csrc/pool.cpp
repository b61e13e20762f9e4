#include "pool.h"
#include <hip/hip_runtime_api.h>
#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <map>
#include <string>
#include <vector>
#include <time.h>

namespace fhelin {

void hip_check(hipError_t e, const char* what) {
    if (e != hipSuccess) throw Error(FHELIN_ERR_HIP, std::string(what) + ": " + hipGetErrorString(e));
}

// ---------------------------------------------------------------- DevicePool
void* DevicePool::raw_malloc(size_t bytes) {
    if (backend_.malloc_fn) return backend_.malloc_fn(bytes);
    void* p = nullptr;
    if (hipMalloc(&p, bytes) != hipSuccess) {
        (void)hipGetLastError();  // the failure is handled by the caller; do not leave it for the next launch check
        return nullptr;
    }
    return p;
}
void DevicePool::raw_free(void* p) {
    if (backend_.free_fn) backend_.free_fn(p);
    else (void)hipFree(p);
}
DevicePool::~DevicePool() {
    for (auto& ln : lane_) {
        for (auto& pk : ln.parked)
            for (int k = 0; k < pk.n_ev; ++k) (void)hipEventDestroy(pk.ev[k]);
        for (auto& sl : ln.slabs)
            if (sl.base) raw_free(sl.base);
    }
    for (hipEvent_t e : spare_events_) (void)hipEventDestroy(e);
}
size_t DevicePool::slabs() const {
    size_t n = 0;
    for (const auto& ln : lane_)
        for (const auto& sl : ln.slabs) n += sl.base != nullptr;
    return n;
}
size_t DevicePool::free_ranges() const {
    size_t n = 0;
    for (const auto& ln : lane_) n += ln.by_size.size();
    return n;
}
void DevicePool::erase_size_entry(Lane& ln, int slab, size_t off, size_t len) {
    auto r = ln.by_size.equal_range(len);
    for (auto it = r.first; it != r.second; ++it)
        if (it->second.first == slab && it->second.second == off) {
            ln.by_size.erase(it);
            return;
        }
    throw Error(FHELIN_ERR_INTERNAL, "DevicePool: free list out of step");
}
// a range goes back into its slab's free list, merged with the free ranges it touches
void DevicePool::insert_free(Lane& ln, int slab, size_t off, size_t len) {
    Slab& sl = ln.slabs[slab];
    auto nxt = sl.free_at.lower_bound(off);
    if (nxt != sl.free_at.begin()) {
        auto prv = std::prev(nxt);
        if (prv->first + prv->second == off) {
            off = prv->first;
            len += prv->second;
            erase_size_entry(ln, slab, prv->first, prv->second);
            sl.free_at.erase(prv);
        }
    }
    if (nxt != sl.free_at.end() && off + len == nxt->first) {
        len += nxt->second;
        erase_size_entry(ln, slab, nxt->first, nxt->second);
        sl.free_at.erase(nxt);
    }
    sl.free_at[off] = len;
    ln.by_size.emplace(len, std::make_pair(slab, off));
}
// one more slab for this lane, large enough for `bytes`: geometric growth, so that a small context stays small and a large one
// reaches the slab size in a few steps
bool DevicePool::grow(Lane& ln, size_t bytes) {
    size_t want = std::max(bytes, std::min(SLAB_MAX, std::max(SLAB_MIN, reserved_)));
    want = (want + (size_t(2) << 20) - 1) & ~((size_t(2) << 20) - 1);
    timespec t0, t1;
    clock_gettime(CLOCK_MONOTONIC, &t0);
    void* p = raw_malloc(want);
    if (!p && want > bytes) {   // not that much left: exactly what is asked for
        want = (bytes + (size_t(2) << 20) - 1) & ~((size_t(2) << 20) - 1);
        p = raw_malloc(want);
    }
    clock_gettime(CLOCK_MONOTONIC, &t1);
    if (!p) return false;
    malloc_calls += 1;
    malloc_bytes += want;
    malloc_ns += (u64)((t1.tv_sec - t0.tv_sec) * 1000000000ll + (t1.tv_nsec - t0.tv_nsec));
    reserved_ += want;
    if (reserved_ > reserved_peak) reserved_peak = reserved_;
    int idx = -1;
    for (size_t i = 0; i < ln.slabs.size(); ++i)
        if (!ln.slabs[i].base) idx = (int)i;      // a slot a trim has emptied
    if (idx < 0) {
        ln.slabs.emplace_back();
        idx = (int)ln.slabs.size() - 1;
    }
    Slab& sl = ln.slabs[idx];
    sl.base = static_cast<char*>(p);
    sl.size = want;
    sl.used = 0;
    sl.free_at.clear();
    insert_free(ln, idx, 0, want);
    return true;
}
void* DevicePool::alloc(size_t bytes) {
    if (bytes == 0) bytes = 256;
    // 256-byte granules for small blocks, 4 KiB above 64 KiB (fewer distinct fragment sizes)
    const size_t gran = bytes > (size_t(64) << 10) ? 4096 : 256;
    bytes = (bytes + gran - 1) & ~(gran - 1);
    Lane& ln = lane_[cur_lane];
    // ranges that were freed under another lane: this lane's stream goes behind that use (no host wait), then they are ordinary
    // free memory of this lane
    if (!ln.parked.empty()) {
        for (auto& pk : ln.parked) {
            for (int k = 0; k < pk.n_ev; ++k) {
                hip_check(hipStreamWaitEvent(lane_stream[cur_lane], pk.ev[k], 0), "hipStreamWaitEvent(pool reuse)");
                spare_events_.push_back(pk.ev[k]);
            }
            insert_free(ln, pk.slab, pk.off, pk.len);
        }
        ln.parked.clear();
    }
    auto it = ln.by_size.lower_bound(bytes);
    if (it == ln.by_size.end()) {
        if (!grow(ln, bytes)) {
            trim();                                            // out of memory: give back what holds nothing, then once more
            if (!grow(ln, bytes)) throw Error(FHELIN_ERR_HIP, "hipMalloc: out of device memory (" + std::to_string(bytes >> 20) + " MiB asked, " +
                                                                  std::to_string(reserved_ >> 20) + " MiB held, " + std::to_string(live_bytes_ >> 20) + " MiB in use)");
        }
        it = ln.by_size.lower_bound(bytes);
    }
    const int slab = it->second.first;
    const size_t off = it->second.second, len = it->first;
    Slab& sl = ln.slabs[slab];
    ln.by_size.erase(it);
    sl.free_at.erase(off);
    if (len > bytes) {
        sl.free_at[off + bytes] = len - bytes;
        ln.by_size.emplace(len - bytes, std::make_pair(slab, off + bytes));
    }
    sl.used += bytes;
    void* p = sl.base + off;
    live_[p] = Live{bytes, cur_lane, slab, off};
    live_bytes_ += bytes;
    if (live_bytes_ > live_peak) live_peak = live_bytes_;
    if (fill_word) fill(p, bytes);
    return p;
}
// the whole rounded block, granule padding included; returns when the words are written: one table upload of the Context is a blocking
// hipMemcpy outside the context's streams, and the knob must not add an ordering question of its own
void DevicePool::fill(void* p, size_t bytes) {
    if (backend_.fill_fn) {
        backend_.fill_fn(p, fill_word, bytes / 4);
    } else {
        hipStream_t s = have_streams ? lane_stream[cur_lane] : nullptr;
        hip_check(hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(p), (int)fill_word, bytes / 4, s), "hipMemsetD32Async(pool fill)");
        hip_check(hipStreamSynchronize(s), "hipStreamSynchronize(pool fill)");
    }
    fill_blocks += 1;
    fill_bytes += bytes;
}
uint32_t DevicePool::parse_fill(const char* text) {
    if (!text || !*text) return 0;
    char* end = nullptr;
    const unsigned long long v = std::strtoull(text, &end, 10);
    if (text[0] < '0' || text[0] > '9' || *end != 0 || v > FILL_MAX)
        throw Error(FHELIN_ERR_ARG, "FHELIN_POOL_FILL must be a decimal word in 0.." + std::to_string(FILL_MAX) + " (0: off), got '" + std::string(text) + "'");
    return (uint32_t)v;
}
void DevicePool::free(void* p, unsigned used_by_lanes) {
    if (!p) return;
    auto it = live_.find(p);
    if (it == live_.end()) throw Error(FHELIN_ERR_STATE, "DevicePool::free of unknown pointer");
    const Live lv = it->second;
    live_.erase(it);
    live_bytes_ -= lv.bytes;
    Lane& ln = lane_[lv.lane];
    ln.slabs[lv.slab].used -= lv.bytes;
    // the lanes whose streams may still have work queued that reads the block, other than the owner (whose own stream order covers it)
    unsigned wait = used_by_lanes;
    if (have_streams && lv.lane != cur_lane) {
        wait |= 1u << cur_lane;
        if (conservative_foreign_free)
            for (int k = 0; k <= n_user_lanes; ++k) wait |= 1u << k;
    }
    wait &= ~(1u << lv.lane);
    if (!have_streams || !wait) {
        insert_free(ln, lv.slab, lv.off, lv.bytes);
        return;
    }
    Parked pk{lv.slab, lv.off, lv.bytes, {}, 0};
    for (int k = 0; k < MAX_LANES; ++k) {
        if (!(wait & (1u << k)) || !lane_stream[k]) continue;
        hipEvent_t ev = nullptr;
        if (!spare_events_.empty()) {
            ev = spare_events_.back();
            spare_events_.pop_back();
        } else {
            hip_check(hipEventCreateWithFlags(&ev, hipEventDisableTiming), "hipEventCreate(pool)");
        }
        hip_check(hipEventRecord(ev, lane_stream[k]), "hipEventRecord(pool free)");
        pk.ev[pk.n_ev++] = ev;
    }
    foreign_frees += 1;
    ln.parked.push_back(pk);
}
void DevicePool::trim() {
    trims += 1;
    if (!backend_.malloc_fn) (void)hipDeviceSynchronize();
    for (auto& ln : lane_) {
        for (auto& pk : ln.parked) {            // the device is idle: parked ranges are plain free memory
            for (int k = 0; k < pk.n_ev; ++k) spare_events_.push_back(pk.ev[k]);
            insert_free(ln, pk.slab, pk.off, pk.len);
        }
        ln.parked.clear();
        for (size_t i = 0; i < ln.slabs.size(); ++i) {
            Slab& sl = ln.slabs[i];
            if (!sl.base || sl.used != 0) continue;
            erase_size_entry(ln, (int)i, 0, sl.size);   // an unused slab is one free range
            raw_free(sl.base);
            reserved_ -= sl.size;
            sl = Slab();
        }
    }
}

// ---------------------------------------------------------------- host self-test of the fill knob
namespace {
constexpr uint32_t SLAB_WORD = 0xA5A5A5A5u;       // what a fresh slab of the host backend holds
size_t g_pool_fill_calls = 0;
void mark_words(void* p, uint32_t w, size_t words) {
    uint32_t* q = static_cast<uint32_t*>(p);
    for (size_t i = 0; i < words; ++i) q[i] = w;
}
void* host_malloc(size_t bytes) {
    void* p = std::malloc(bytes);
    if (p) mark_words(p, SLAB_WORD, bytes / 4);
    return p;
}
void host_free(void* p) { std::free(p); }
void host_fill(void* p, uint32_t w, size_t words) {
    g_pool_fill_calls += 1;
    mark_words(p, w, words);
}
}  // namespace
void pool_fill_selftest(uint64_t seed, int n_ops, uint32_t w, uint64_t* out, int cap) {
    if (!out || cap < 6 || n_ops < 1) throw Error(FHELIN_ERR_ARG, "pool fill selftest: need room for 6 results");
    if (w > DevicePool::FILL_MAX) throw Error(FHELIN_ERR_ARG, "pool fill selftest: w above the cap");
    DevicePool::Backend be;
    be.malloc_fn = host_malloc;
    be.free_fn = host_free;
    be.fill_fn = host_fill;
    g_pool_fill_calls = 0;
    DevicePool pool(be);
    pool.fill_word = w;
    struct Blk { size_t rounded; uint32_t mark; };
    std::map<char*, Blk> live;            // address-ordered: a fill that overruns its block lands in a neighbour first
    std::vector<char*> order;
    u64 x = seed * 0x9E3779B97F4A7C15ull + 1;
    auto rnd = [&]() {
        x ^= x << 13;
        x ^= x >> 7;
        x ^= x << 17;
        return x;
    };
    auto fail = [](const char* what, int op) { throw Error(FHELIN_ERR_INTERNAL, std::string("pool fill selftest: ") + what + " (op " + std::to_string(op) + ")"); };
    // a block's marker is above FILL_MAX and unique among the blocks ever handed out: neither a fill nor a neighbour can pass for it
    uint32_t next_mark = 0x10000;
    u64 blocks = 0, rounded_sum = 0, big = 0;
    size_t live_bytes = 0;
    auto check_block = [&](const char* p, const Blk& b, int op) {
        const uint32_t* q = reinterpret_cast<const uint32_t*>(p);
        for (size_t i = 0; i < b.rounded / 4; ++i)
            if (q[i] != b.mark) fail("a live block's contents changed", op);
    };
    auto check_all = [&](int op) {
        for (const auto& kv : live) check_block(kv.first, kv.second, op);
    };
    for (int op = 0; op < n_ops; ++op) {
        // at most 48 MiB live: past the first slab (32 MiB) more than once, small enough for a sanitized run
        const bool do_alloc = live.empty() || (live_bytes < (size_t(48) << 20) && (rnd() % 100) < 55);
        if (do_alloc) {
            size_t bytes;
            switch (rnd() % 6) {
                case 0: bytes = rnd() % 300; break;                                   // 0 (handed out as one granule) .. just past one
                case 1: bytes = 256 + rnd() % 8192; break;
                case 2: bytes = (size_t(64) << 10) - 300 + rnd() % 600; break;        // around the threshold between the granule classes
                case 3: bytes = (size_t(64) << 10) + 1 + rnd() % (size_t(1) << 20); break;
                case 4: bytes = (size_t(1) << 20) * (1 + rnd() % 12) + rnd() % 4096; break;
                default: bytes = 4 * (1 + rnd() % 4096); break;
            }
            const size_t b0 = bytes ? bytes : 256, gran = b0 > (size_t(64) << 10) ? 4096 : 256;
            const size_t rounded = (b0 + gran - 1) & ~(gran - 1);
            const size_t before = pool.bytes_live();
            char* p = static_cast<char*>(pool.alloc(bytes));
            if (pool.bytes_live() - before != rounded) fail("rounded size differs from the granule rule", op);
            const uint32_t* q = reinterpret_cast<const uint32_t*>(p);
            for (size_t i = 0; i < rounded / 4; ++i) {
                if (w ? q[i] != w : !(q[i] == SLAB_WORD || (q[i] >= 0x10000 && q[i] < next_mark)))     // off: what the slab or an earlier owner left
                    fail(w ? "a word of the handed-out block is not w" : "a handed-out block was written with the knob off", op);
            }
            // the fill stayed inside its block: both address neighbours word for word at every hand-out, every live block every 64th
            // operation and at the end (and each block once more when it is freed)
            auto nx = live.lower_bound(p);
            if (nx != live.end()) {
                if (p + rounded > nx->first) fail("block overlaps its successor", op);
                check_block(nx->first, nx->second, op);
            }
            if (nx != live.begin()) {
                auto pv = std::prev(nx);
                if (pv->first + pv->second.rounded > p) fail("block overlaps its predecessor", op);
                check_block(pv->first, pv->second, op);
            }
            const uint32_t mark = next_mark++;
            mark_words(p, mark, rounded / 4);
            live[p] = Blk{rounded, mark};
            order.push_back(p);
            live_bytes += rounded;
            blocks += 1;
            rounded_sum += rounded;
            big += gran == 4096;
        } else {
            const size_t k = rnd() % order.size();
            char* p = order[k];
            order[k] = order.back();
            order.pop_back();
            check_block(p, live[p], op);
            live_bytes -= live[p].rounded;
            live.erase(p);
            pool.free(p);
        }
        if (op % 64 == 63) check_all(op);
        if (!w && (pool.fill_blocks || pool.fill_bytes || g_pool_fill_calls)) fail("a fill ran with the knob off", op);
    }
    check_all(n_ops);
    if (w && g_pool_fill_calls != blocks) fail("fills and hand-outs differ in number", n_ops);
    out[0] = blocks;
    out[1] = rounded_sum;
    out[2] = pool.fill_blocks;
    out[3] = pool.fill_bytes;
    out[4] = pool.malloc_calls;
    out[5] = big;
    for (char* p : order) pool.free(p);
    if (pool.free_ranges() != pool.slabs() || pool.bytes_live() != 0) fail("freeing everything did not coalesce to one range per slab", n_ops);
    pool.trim();
    if (pool.bytes_reserved() != 0) fail("trim kept a slab", n_ops);
}

}  // namespace fhelin
