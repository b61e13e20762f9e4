// Device memory arena (DevicePool), its scoped owner (Scratch) and the error type they throw.  Kept apart from the Context so that the
// allocator's logic compiles into a stand-alone host program (tests/shim/pool_fill_host.cpp) as well as into the library.
#pragma once
#include <cstddef>
#include <cstdint>
#include <map>
#include <stdexcept>
#include <string>
#include <unordered_map>
#include <vector>
#include <hip/hip_runtime_api.h>
#include "../../include/fhelin.h"  // status codes

namespace fhelin {

typedef uint64_t u64;

struct Error : std::runtime_error {
    int code;
    Error(int c, const std::string& m) : std::runtime_error(m), code(c) {}
};

void hip_check(hipError_t e, const char* what);

// Device memory arena (sized for the 288 GB of an MI355X: the key set, the resident inputs and the intermediates of a batched pass
// share it).  Memory comes from the driver in SLABS (few, large hipMalloc calls: geometric growth up to 8 GiB a slab, or the
// request itself when that is larger) and is handed out by BEST FIT from an address-ordered free list with coalescing: a freed
// block merges with its free neighbours, so the ciphertext blocks of one stage (say 6 GB of unwrapped rows) are carved up again by
// the next one, whatever its sizes.  (Rounds 1-3 cached freed blocks by exact size class: with many samples per pass the idle
// lists held 1.6 x the bytes in use and the device ran out of memory - every time at the price of a device-wide synchronisation.)
// Work is stream-ordered, so a freed block can be handed out again immediately - to the SAME stream.  With several lanes (streams)
// every lane has its own slabs and free list; a block that is freed while ANOTHER lane is current (a worker lane's result consumed
// and released on the main stream, or the reverse) may still be read by work queued on that other lane's stream: the free records
// an event there, and the owner lane's stream waits for it before the range goes back into the owner's free list.
// The backend (hipMalloc / hipFree) is replaceable: the allocator's logic is unit-tested on the host (fhelin_debug_pool_selftest).
class DevicePool {
public:
    static constexpr int MAX_LANES = 5;  // lane 0 = main stream
    static constexpr size_t SLAB_MAX = size_t(8) << 30, SLAB_MIN = size_t(32) << 20;
    struct Backend {
        void* (*malloc_fn)(size_t) = nullptr;   // null: hipMalloc / hipFree
        void (*free_fn)(void*) = nullptr;
        // fill `words` 32-bit words at p with w and return once they are written; null: hipMemsetD32Async on the current lane's
        // stream, then a wait for that stream
        void (*fill_fn)(void* p, uint32_t w, size_t words) = nullptr;
    };
    DevicePool() = default;
    explicit DevicePool(const Backend& b) : backend_(b) {}
    ~DevicePool();
    void* alloc(size_t bytes);
    // used_by_lanes: lanes (bit k) whose queued work may still read the block besides the current one (a plaintext encoding shared by
    // the lanes of a pass): the owner lane reuses the range only behind all of them
    void free(void* p, unsigned used_by_lanes = 0);
    // between fhelin_ctx_lanes_fork and _join the caller's lanes run side by side and a handle may be dropped (a host language's garbage
    // collection) while ANY lane is current: a free under a foreign lane then waits for every lane, not only the current one
    bool conservative_foreign_free = false;
    int n_user_lanes = 0;
    void trim();                                // hand slabs that hold nothing back to the driver (synchronises the device first)
    size_t bytes_reserved() const { return reserved_; }
    size_t bytes_live() const { return live_bytes_; }
    size_t slabs() const;
    size_t free_ranges() const;
    int cur_lane = 0;
    hipStream_t lane_stream[MAX_LANES] = {};   // set by the Context: the stream each lane launches on (lane 0 = main stream)
    bool have_streams = false;
    // growth diagnostics (fhelin_stats slots 9..11): slabs obtained from hipMalloc, their bytes, host time spent inside hipMalloc
    u64 malloc_calls = 0, malloc_bytes = 0, malloc_ns = 0;
    u64 foreign_frees = 0;
    u64 trims = 0;                              // out-of-memory events: empty slabs handed back (a device-wide synchronisation each)
    size_t live_peak = 0, reserved_peak = 0;    // high-water marks: bytes in use, bytes held from the driver
    // FHELIN_POOL_FILL=<w> (a test aid, off by default; DESIGN.md "Pool fill"): every block is handed out with w in each 32-bit word of
    // its ROUNDED size, written on the current lane's stream, and alloc returns only when the fill has finished - a result that depends on
    // memory nobody wrote in this call then depends on w.  w <= FILL_MAX keeps a stale word that is read as an index, a limb id or a
    // count inside every table of every accepted ring (N >= 4096).  Slabs are not filled when they are obtained.
    static constexpr uint32_t FILL_MAX = 4095;
    uint32_t fill_word = 0;                     // 0: off
    u64 fill_blocks = 0, fill_bytes = 0;        // blocks and bytes filled (fhelin_debug_pool_fill_stats)
    // the knob's text -> w; unset, empty or "0": 0 (off); anything that is not a decimal number in 1..FILL_MAX: Error(FHELIN_ERR_ARG)
    static uint32_t parse_fill(const char* text);
private:
    struct Slab {
        char* base = nullptr;
        size_t size = 0, used = 0;
        std::map<size_t, size_t> free_at;       // offset -> length of the free ranges, address-ordered
    };
    struct Live { size_t bytes; int lane; int slab; size_t off; };
    struct Parked { int slab; size_t off, len; hipEvent_t ev[MAX_LANES]; int n_ev; };   // freed while other lanes may read it: waits for their events
    struct Lane {
        std::vector<Slab> slabs;
        std::multimap<size_t, std::pair<int, size_t>> by_size;      // length -> (slab, offset): best fit
        std::vector<Parked> parked;
    };
    Backend backend_;
    Lane lane_[MAX_LANES];
    std::unordered_map<void*, Live> live_;
    std::vector<hipEvent_t> spare_events_;
    size_t reserved_ = 0, live_bytes_ = 0;
    void insert_free(Lane& ln, int slab, size_t off, size_t len);
    void erase_size_entry(Lane& ln, int slab, size_t off, size_t len);
    bool grow(Lane& ln, size_t bytes);
    void* raw_malloc(size_t bytes);
    void fill(void* p, size_t bytes);
    void raw_free(void* p);
};

// Owner of one block of pool scratch: freed when it goes out of scope (also when an exception unwinds through it), by reset()
// for an early free, handed on by release().  An empty one frees nothing.  Two rules keep the pool's behaviour predictable:
// the scope closes (or reset() is called) where the block is no longer needed - a block held across a later allocation raises the
// pool's peak - and under the lane the block was allocated under, because a free under a foreign lane parks the block behind an
// event (DevicePool::free).
template <class T>
class Scratch {
public:
    Scratch() = default;
    Scratch(DevicePool& pool, size_t count) : pool_(&pool), p_(static_cast<T*>(pool.alloc(count * sizeof(T)))) {}
    Scratch(Scratch&& o) noexcept : pool_(o.pool_), p_(o.release()) {}
    Scratch& operator=(Scratch&& o) noexcept {
        if (this != &o) {
            drop();
            pool_ = o.pool_;
            p_ = o.release();
        }
        return *this;
    }
    Scratch(const Scratch&) = delete;
    Scratch& operator=(const Scratch&) = delete;
    ~Scratch() { drop(); }
    operator T*() const& { return p_; }
    operator T*() && = delete;   // a temporary's block would be gone before the pointer is used
    T* get() const { return p_; }
    void reset() {               // early free; errors surface as from DevicePool::free
        if (T* p = release()) pool_->free(p);
    }
    T* release() noexcept {
        T* p = p_;
        p_ = nullptr;
        return p;
    }
private:
    void drop() noexcept {
        try { reset(); } catch (...) {}
    }
    DevicePool* pool_ = nullptr;
    T* p_ = nullptr;
};

// Host self-test of the fill knob (fhelin_debug_pool_fill_selftest, tests/shim/pool_fill_host.cpp): a pool over host malloc with a host
// fill function runs n_ops seeded allocations and frees - both granule classes, splits, coalescing, growth past one slab - and checks at
// every hand-out that each word of the rounded block is w, and that every other live block still holds its own marker up to its last
// rounded byte; w == 0: that nothing is written at all.  out (cap >= 6): [0] blocks handed out, [1] the sum of their rounded sizes,
// [2] the pool's fill_blocks, [3] its fill_bytes, [4] slabs obtained, [5] hand-outs at the 4 KiB granule.  Throws Error on a violation.
void pool_fill_selftest(uint64_t seed, int n_ops, uint32_t w, uint64_t* out, int cap);

}  // namespace fhelin
