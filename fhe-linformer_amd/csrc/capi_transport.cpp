// extern "C" boundary, part 13: device transport (include/fhelin.h "Device transport": frames, metadata and the stream contract are
// documented there).  A set of ciphertexts goes into (comes out of) the frames of ONE device buffer: one pack table for every limb
// vector of the set through pinned staging and one launch of the packing kernels (kernels_pack.hip) - or one device copy per raw
// frame - and the ordering against the caller's stream is a pair of events, not a host synchronisation per ciphertext.
#include "../../include/fhelin.h"
#include <hip/hip_runtime.h>
#include <cmath>
#include <map>
#include <vector>
#include "capi_internal.h"
#include "kernels_keys.h"
#include "kernels_pack.h"

using namespace fhelin;

namespace {

constexpr int META = 8;   // doubles per metadata row: npoly, ell, deg, slots, scale hi, scale lo, payload bytes, format

// payload bytes of one component's first `ell` limb vectors
size_t limb_bytes(const Context& x, int ell, int format) {
    if (format == 0) return (size_t)ell * x.N * 8;
    size_t words = 0;
    for (int l = 0; l < ell; ++l) {
        const int w = pack_width(x.moduli[l]);
        if (w < PACK_MIN_WIDTH || w > PACK_MAX_WIDTH) throw Error(FHELIN_ERR_ARG, "device transport: a modulus outside 20..60 bits");
        words += pack_words(x.N, w);
    }
    return words * 8;
}

void check_format(int32_t format) {
    if (format != 0 && format != 1) throw Error(FHELIN_ERR_ARG, "device transport: format must be 0 (raw) or 1 (packed)");
}

void check_buffer(const uint8_t* d_buf, size_t stride) {
    if (stride == 0 || stride % 16) throw Error(FHELIN_ERR_ARG, "device transport: stride_bytes must be a positive multiple of 16");
    if ((uintptr_t)d_buf % 16) throw Error(FHELIN_ERR_ARG, "device transport: the buffer must be 16-byte aligned");
}

// the handles of a frame set: none null, none wrapped; everything deferred among them evaluated together
void force_set(fhelin_ctx* c, const fhelin_ct* const* cts, int n, const char* who) {
    for (int i = 0; i < n; ++i) {
        if (!cts[i]) throw Error(FHELIN_ERR_ARG, std::string(who) + ": null ciphertext handle in array");
        if (cts[i]->p && cts[i]->p->wrapped())
            throw Error(FHELIN_ERR_ARG, std::string(who) + ": handle " + std::to_string(i) + " is a wrapped input ciphertext (unwrap it first)");
    }
    c->ctx.require_device();
    force_many(c, cts, n);
    for (int i = 0; i < n; ++i) force(c, cts[i]);   // every handle now points at its value
}

size_t frame_bytes_of(const Context& x, const Ciphertext& ct, int format, const char* who, int i) {
    if (ct.wrapped()) throw Error(FHELIN_ERR_ARG, std::string(who) + ": handle " + std::to_string(i) + " is a wrapped input ciphertext");
    if (ct.npoly < 2 || ct.npoly > 3) throw Error(FHELIN_ERR_ARG, std::string(who) + ": handle " + std::to_string(i) + " has other than 2 or 3 components");
    return (size_t)ct.npoly * limb_bytes(x, ct.ell, format);
}

// the table of a pack / unpack launch, through the pinned staging ring (no stream drain), in pieces of at most one staging slot
void upload_table(Context& x, PackEntry* d_tab, const std::vector<PackEntry>& tab) {
    static_assert(sizeof(PackEntry) == 24, "a table entry is three words");
    const size_t per = x.stage_words / 3;   // entries per piece
    for (size_t lo = 0; lo < tab.size(); lo += per) {
        const size_t cnt = std::min(per, tab.size() - lo);
        x.upload_async(reinterpret_cast<u64*>(d_tab + lo), reinterpret_cast<const u64*>(tab.data() + lo), 3 * cnt);
    }
}

hipEvent_t transport_event(Context& x) {
    if (!x.transport_ev) hip_check(hipEventCreateWithFlags(&x.transport_ev, hipEventDisableTiming), "hipEventCreate(transport)");
    return x.transport_ev;
}
// The caller's stream of a call.  NULL means none (the call synchronises the host once); the legacy default stream, whose own handle
// is NULL, is named by hipStreamLegacy and handed to the runtime as the NULL it is.
struct Caller {
    bool given;
    hipStream_t s;
    explicit Caller(void* hip_stream) : given(hip_stream != nullptr), s(hip_stream == (void*)hipStreamLegacy ? nullptr : (hipStream_t)hip_stream) {}
};
// the library's stream behind everything issued on the caller's stream so far
void wait_for_caller(Context& x, const Caller& caller) {
    if (!caller.given || caller.s == x.stream) return;
    hipEvent_t ev = transport_event(x);
    hip_check(hipEventRecord(ev, caller.s), "hipEventRecord(caller stream)");
    hip_check(hipStreamWaitEvent(x.stream, ev, 0), "hipStreamWaitEvent(library behind caller)");
}
// the caller's stream behind the library's last launch; without a stream of the caller's, the call's one host synchronisation
void hand_over(Context& x, const Caller& caller, bool synced) {
    if (!caller.given) {
        if (!synced) x.sync();
        return;
    }
    if (caller.s == x.stream) return;
    hipEvent_t ev = transport_event(x);
    hip_check(hipEventRecord(ev, x.stream), "hipEventRecord(library stream)");
    hip_check(hipStreamWaitEvent(caller.s, ev, 0), "hipStreamWaitEvent(caller behind library)");
}

// a metadata entry that must be an integer in [lo, hi]
int meta_int(double v, int lo, int hi, const std::string& at, const char* what) {
    if (!(v >= lo && v <= hi) || v != std::floor(v)) throw Error(FHELIN_ERR_ARG, at + what);
    return (int)v;
}

struct Frame {
    int npoly = 0, ell = 0, deg = 0, slots = 0, format = 0;
    long double scale = 0;
};

}  // namespace

extern "C" {

int fhelin_debug_sync_count(fhelin_ctx* c, uint64_t* out) {
    if (!c || !out) return capi_fail(FHELIN_ERR_ARG, "null argument");
    *out = c->ctx.sync_count;
    return FHELIN_OK;
}

int fhelin_debug_ct_addr(const fhelin_ct* ct, uint64_t* data, uint64_t* block) {
    if (!ct || !ct->p || !data || !block) return capi_fail(FHELIN_ERR_ARG, "null argument (or a deferred handle)");
    *data = (uint64_t)(uintptr_t)ct->p->d;
    *block = ct->p->block ? (uint64_t)(uintptr_t)ct->p->block->d : 0;
    return FHELIN_OK;
}

int fhelin_ct_frame_bytes(fhelin_ctx* c, const fhelin_ct* const* cts, int32_t n, int32_t format, size_t* bytes_each, size_t* max_bytes) {
    if (!c || n < 0 || (n > 0 && !cts)) return capi_fail(FHELIN_ERR_ARG, "null argument");
    FHELIN_TRY
    check_format(format);
    if (max_bytes) *max_bytes = 0;
    if (n == 0) return FHELIN_OK;
    force_set(c, cts, n, "frame_bytes");
    size_t most = 0;
    for (int i = 0; i < n; ++i) {
        const size_t b = frame_bytes_of(c->ctx, *cts[i]->p, format, "frame_bytes", i);
        if (bytes_each) bytes_each[i] = b;
        most = std::max(most, b);
    }
    if (max_bytes) *max_bytes = most;
    FHELIN_CATCH
}

int fhelin_ct_export_device_many(fhelin_ctx* c, const fhelin_ct* const* cts, int32_t n, int32_t format, uint8_t* d_buf,
                                 size_t stride_bytes, size_t cap_bytes, double* meta, void* hip_stream) {
    if (!c || n < 0) return capi_fail(FHELIN_ERR_ARG, "null argument");
    if (n == 0) return FHELIN_OK;
    if (!cts || !d_buf || !meta) return capi_fail(FHELIN_ERR_ARG, "null argument");
    FHELIN_TRY
    // 1. what can be said without looking at a handle
    check_format(format);
    check_buffer(d_buf, stride_bytes);
    if (cap_bytes / stride_bytes < (size_t)n) throw Error(FHELIN_ERR_ARG, "export_device_many: cap_bytes is below n * stride_bytes");
    // 2. the handles: deferred ones evaluated together, every frame against the stride
    force_set(c, cts, n, "export_device_many");
    Context& x = c->ctx;
    if (format == 1 && x.N % 4096) throw Error(FHELIN_ERR_ARG, "export_device_many: packed frames need a ring dimension of at least 2^12");
    std::vector<size_t> bytes(n);
    size_t n_vec = 0;
    for (int i = 0; i < n; ++i) {
        bytes[i] = frame_bytes_of(x, *cts[i]->p, format, "export_device_many", i);
        if (bytes[i] > stride_bytes)
            throw Error(FHELIN_ERR_ARG, "export_device_many: frame " + std::to_string(i) + " needs " + std::to_string(bytes[i]) +
                                            " bytes, above stride_bytes");
        n_vec += (size_t)cts[i]->p->npoly * cts[i]->p->ell;
    }
    // 3. every handle is a terminal of the level plan, as in fhelin_ct_export_device
    CtVec ps(n);
    for (int i = 0; i < n; ++i) {
        if (c->plan.live(cts[i]->node, cts[i]->node_epoch)) c->plan.terminal(cts[i]->node, 2);
        ps[i] = ct_in(c, cts[i]);
        c->plan.check_terminal(*ps[i], 2);
    }
    const Caller caller(hip_stream);
    wait_for_caller(x, caller);   // whatever still reads the buffer on the caller's stream comes first
    const size_t N = x.N;
    if (format == 0) {
        for (int i = 0; i < n; ++i)
            hip_check(hipMemcpyAsync(d_buf + (size_t)i * stride_bytes, ps[i]->d, bytes[i], hipMemcpyDeviceToDevice, x.stream), "export_device_many copy");
    } else {
        std::vector<int> width(x.L + 1);
        for (int l = 0; l <= x.L; ++l) width[l] = pack_width(x.moduli[l]);
        std::vector<PackEntry> tab;
        tab.reserve(n_vec);
        for (int i = 0; i < n; ++i) {
            const Ciphertext& ct = *ps[i];
            u64* at = reinterpret_cast<u64*>(d_buf + (size_t)i * stride_bytes);
            for (int v = 0; v < ct.npoly * ct.ell; ++v) {
                const int w = width[v % ct.ell];
                tab.push_back(PackEntry{ct.d + (size_t)v * N, at, (u32)w, 0});
                at += pack_words(N, w);
            }
        }
        Scratch<PackEntry> d_tab = x.scratch<PackEntry>(tab.size());
        upload_table(x, d_tab, tab);
        launch_pack_residues(d_tab, (int)tab.size(), x.N, x.stream);
        hip_check(hipGetLastError(), "export_device_many pack");
    }
    for (int i = 0; i < n; ++i) {
        const Ciphertext& ct = *ps[i];
        double* m = meta + (size_t)META * i;
        m[0] = ct.npoly;
        m[1] = ct.ell;
        m[2] = ct.deg;
        m[3] = ct.slots;
        m[4] = (double)ct.scale;                                // as fhelin_ct_scale
        m[5] = (double)(ct.scale - (long double)m[4]);
        m[6] = (double)bytes[i];
        m[7] = format;
    }
    hand_over(x, caller, false);
    FHELIN_CATCH
}

int fhelin_ct_import_device_many(fhelin_ctx* c, const uint8_t* d_buf, size_t stride_bytes, const double* meta, int32_t n, int32_t check,
                                 void* hip_stream, fhelin_ct** outs) {
    if (!c || n < 0) return capi_fail(FHELIN_ERR_ARG, "null argument");
    if (n == 0) return FHELIN_OK;
    if (!d_buf || !meta || !outs) return capi_fail(FHELIN_ERR_ARG, "null argument");
    FHELIN_TRY
    Context& x = c->ctx;
    // 1. every row of the metadata, on the host, before anything is allocated or launched
    check_buffer(d_buf, stride_bytes);
    std::vector<Frame> fr(n);
    bool any_packed = false;
    for (int i = 0; i < n; ++i) {
        const double* m = meta + (size_t)META * i;
        const std::string at = "import_device_many: frame " + std::to_string(i) + ": ";
        Frame& f = fr[i];
        f.npoly = meta_int(m[0], 2, 3, at, "npoly must be 2 or 3");
        f.ell = meta_int(m[1], 1, x.L + 1, at, "ell outside 1..n_q");
        f.deg = meta_int(m[2], 1, 2, at, "deg must be 1 or 2");
        f.slots = meta_int(m[3], 0, x.N / 2, at, "slots outside 0..N/2");   // 0: as fhelin_ct_import leaves it (the context's default)
        if (f.slots & (f.slots - 1)) throw Error(FHELIN_ERR_ARG, at + "slots must be a power of two");
        if (!(std::isfinite(m[4]) && m[4] > 0 && std::isfinite(m[5]) && std::fabs(m[5]) <= std::ldexp(m[4], -52)))
            throw Error(FHELIN_ERR_ARG, at + "bad scale");
        f.scale = (long double)m[4] + (long double)m[5];
        f.format = meta_int(m[7], 0, 1, at, "format must be 0 (raw) or 1 (packed)");
        const size_t want = (size_t)f.npoly * limb_bytes(x, f.ell, f.format);
        if (m[6] != (double)want)
            throw Error(FHELIN_ERR_ARG, at + "payload_bytes does not match the context's moduli (" + std::to_string(want) + " expected)");
        if (want > stride_bytes) throw Error(FHELIN_ERR_ARG, at + "payload_bytes is above stride_bytes");
        any_packed |= f.format == 1;
    }
    x.require_device();
    if (any_packed && x.N % 4096) throw Error(FHELIN_ERR_ARG, "import_device_many: packed frames need a ring dimension of at least 2^12");
    // 2. one batch allocation per (components, limbs), rows in frame order
    std::map<std::pair<int, int>, std::vector<int>> groups;
    for (int i = 0; i < n; ++i) groups[{fr[i].npoly, fr[i].ell}].push_back(i);
    std::vector<CtPtr> cts(n);
    size_t n_vec = 0;
    for (auto& g : groups) {
        std::vector<CtPtr> b = c->ev.new_ct_batch((int)g.second.size(), g.first.first, g.first.second, 1, 1.0L, 1);
        for (size_t k = 0; k < g.second.size(); ++k) {
            const Frame& f = fr[g.second[k]];
            b[k]->deg = f.deg;
            b[k]->slots = f.slots;
            b[k]->scale = f.scale;
            cts[g.second[k]] = b[k];
            if (f.format == 1) n_vec += (size_t)f.npoly * f.ell;
        }
    }
    // 3. behind the producer of the frames; raw frames are copies, every packed vector goes through one unpack launch
    const Caller caller(hip_stream);
    wait_for_caller(x, caller);
    const size_t N = x.N;
    std::vector<PackEntry> tab;
    tab.reserve(n_vec);
    std::vector<int> width(x.L + 1);
    for (int l = 0; l <= x.L; ++l) width[l] = pack_width(x.moduli[l]);
    for (int i = 0; i < n; ++i) {
        const Frame& f = fr[i];
        const uint8_t* src = d_buf + (size_t)i * stride_bytes;
        if (f.format == 0) {
            hip_check(hipMemcpyAsync(cts[i]->d, src, cts[i]->words() * 8, hipMemcpyDeviceToDevice, x.stream), "import_device_many copy");
            continue;
        }
        const u64* at = reinterpret_cast<const u64*>(src);
        for (int v = 0; v < f.npoly * f.ell; ++v) {
            const int w = width[v % f.ell];
            tab.push_back(PackEntry{at, cts[i]->d + (size_t)v * N, (u32)w, 0});
            at += pack_words(N, w);
        }
    }
    Scratch<PackEntry> d_tab;
    if (!tab.empty()) {
        d_tab = x.scratch<PackEntry>(tab.size());
        upload_table(x, d_tab, tab);
        launch_unpack_residues(d_tab, (int)tab.size(), x.N, x.stream);
        hip_check(hipGetLastError(), "import_device_many unpack");
    }
    // 4. the range check of the other loaders over each shape's block (its vectors are contiguous), at most 65535 vectors a launch;
    // its download needs the host: the call's one synchronisation
    bool synced = false;
    if (check) {
        if (x.N % 4096) throw Error(FHELIN_ERR_ARG, "import_device_many: the range check needs a ring dimension of at least 2^12");
        size_t total = 0, most = 0;
        for (auto& g : groups) {
            const size_t per = (size_t)g.first.first * g.first.second, rows = std::max<size_t>(1, 65535 / per);
            total += g.second.size() * per;
            most = std::max(most, std::min(rows, g.second.size()) * per);
        }
        Scratch<u64> part = x.scratch<u64>(key_digest_scratch_words(x.N, (int)most));
        Scratch<u64> dg = x.scratch<u64>(2 * total);
        std::vector<size_t> dg_at(n);
        size_t v0 = 0;
        for (auto& g : groups) {
            const int ell = g.first.second;
            const size_t per = (size_t)g.first.first * ell, rows = std::max<size_t>(1, 65535 / per);
            for (size_t lo = 0; lo < g.second.size(); lo += rows) {
                const size_t cnt = std::min(rows, g.second.size() - lo);
                launch_key_digest(x.dt, cts[g.second[lo]]->d, (int)(cnt * per), 0, ell, part, dg + 2 * v0, x.stream);
                for (size_t k = 0; k < cnt; ++k) dg_at[g.second[lo + k]] = v0 + k * per;
                v0 += cnt * per;
            }
        }
        hip_check(hipGetLastError(), "import_device_many range check");
        std::vector<u64> h(2 * total);
        hip_check(hipMemcpyAsync(h.data(), dg, h.size() * 8, hipMemcpyDeviceToHost, x.stream), "range flags download");
        x.sync();
        synced = true;
        for (int i = 0; i < n; ++i)
            for (size_t v = 0; v < (size_t)fr[i].npoly * fr[i].ell; ++v)
                if (!h[2 * (dg_at[i] + v) + 1])
                    throw Error(FHELIN_ERR_ARG, "import_device_many: frame " + std::to_string(i) + " holds a residue not below its modulus (range check)");
    }
    hand_over(x, caller, synced);
    for (int i = 0; i < n; ++i) outs[i] = wrap(c, cts[i]);   // imported: not a level-plan source, never lowered
    FHELIN_CATCH
}

}  // extern "C"
