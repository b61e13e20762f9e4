// extern "C" boundary, part 13: device transport (include/fhelin.h "Device transport": frames, metadata and the stream contract are
// documented there).  A set of ciphertexts goes into (comes out of) the frames of ONE device buffer: one pack table for every limb
// vector of the set through pinned staging and one launch of the packing kernels (kernels_pack.hip) - or one device copy per raw
// frame - and the ordering against the caller's stream is a pair of events, not a host synchronisation per ciphertext.  Widths, the
// pack table and its upload, allocation by shape and the range run are wire.h's, shared with the blob formats; the metadata rows and
// the stream hand-off are this file's own.
#include "../../include/fhelin.h"
#include <hip/hip_runtime.h>
#include <cmath>
#include <vector>
#include "capi_internal.h"
#include "wire.h"

using namespace fhelin;

namespace {

constexpr int META = 8;   // doubles per metadata row: npoly, ell, deg, slots, scale hi, scale lo, payload bytes, format

// payload bytes of one component's first `ell` limb vectors
size_t limb_bytes(const Context& x, int ell, int format) {
    return 8 * (format == 0 ? (size_t)ell * x.N : limb_widths(x, 0, ell, "device transport"));
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
    int max_ell = 0;
    for (int i = 0; i < n; ++i) {
        bytes[i] = frame_bytes_of(x, *cts[i]->p, format, "export_device_many", i);
        if (bytes[i] > stride_bytes)
            throw Error(FHELIN_ERR_ARG, "export_device_many: frame " + std::to_string(i) + " needs " + std::to_string(bytes[i]) +
                                            " bytes, above stride_bytes");
        n_vec += (size_t)cts[i]->p->npoly * cts[i]->p->ell;
        max_ell = std::max(max_ell, cts[i]->p->ell);
    }
    // 3. every handle is a terminal of the level plan, as in fhelin_ct_export_device
    CtVec ps(n);
    for (int i = 0; i < n; ++i) ps[i] = terminal_in(c, cts[i]);
    const Caller caller(hip_stream);
    wait_for_caller(x, caller);   // whatever still reads the buffer on the caller's stream comes first
    if (format == 0) {
        for (int i = 0; i < n; ++i)
            hip_check(hipMemcpyAsync(d_buf + (size_t)i * stride_bytes, ps[i]->d, bytes[i], hipMemcpyDeviceToDevice, x.stream), "export_device_many copy");
    } else {
        std::vector<int> width;
        limb_widths(x, 0, max_ell, "device transport", &width);
        std::vector<PackEntry> tab;
        tab.reserve(n_vec);
        for (int i = 0; i < n; ++i)
            pack_rows(tab, x.N, ps[i]->d, (size_t)ps[i]->npoly * ps[i]->ell, width.data(), ps[i]->ell,
                      reinterpret_cast<u64*>(d_buf + (size_t)i * stride_bytes), false);
        Scratch<PackEntry> d_tab = upload_pack_table(x, tab);
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
    int packed_ell = 0;   // most limbs of a packed frame
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
        if (f.format == 1) packed_ell = std::max(packed_ell, f.ell);
    }
    x.require_device();
    if (packed_ell && x.N % 4096) throw Error(FHELIN_ERR_ARG, "import_device_many: packed frames need a ring dimension of at least 2^12");
    // 2. one batch allocation per (components, limbs), rows in frame order
    std::vector<std::pair<int, int>> shape(n);
    for (int i = 0; i < n; ++i) shape[i] = {fr[i].npoly, fr[i].ell};
    ShapeBatch sb(c, shape);
    const std::vector<CtPtr>& cts = sb.cts;
    for (int i = 0; i < n; ++i) {
        cts[i]->deg = fr[i].deg;
        cts[i]->slots = fr[i].slots;
        cts[i]->scale = fr[i].scale;
    }
    // 3. behind the producer of the frames; raw frames are copies, every packed vector goes through one unpack launch
    const Caller caller(hip_stream);
    wait_for_caller(x, caller);
    std::vector<PackEntry> tab;
    std::vector<int> width;
    limb_widths(x, 0, packed_ell, "device transport", &width);
    for (int i = 0; i < n; ++i) {
        const Frame& f = fr[i];
        uint8_t* src = const_cast<uint8_t*>(d_buf) + (size_t)i * stride_bytes;   // read only: the source side of an unpack entry
        if (f.format == 0)
            hip_check(hipMemcpyAsync(cts[i]->d, src, cts[i]->words() * 8, hipMemcpyDeviceToDevice, x.stream), "import_device_many copy");
        else
            pack_rows(tab, x.N, cts[i]->d, (size_t)f.npoly * f.ell, width.data(), f.ell, reinterpret_cast<u64*>(src), true);
    }
    Scratch<PackEntry> d_tab;
    if (!tab.empty()) {
        d_tab = upload_pack_table(x, tab);
        launch_unpack_residues(d_tab, (int)tab.size(), x.N, x.stream);
        hip_check(hipGetLastError(), "import_device_many unpack");
    }
    // 4. the range check of the other loaders over each shape's block (its vectors are contiguous); its download needs the host: the
    // call's one synchronisation
    bool synced = false;
    if (check) {
        if (x.N % 4096) throw Error(FHELIN_ERR_ARG, "import_device_many: the range check needs a ring dimension of at least 2^12");
        DigestRun run(x, sb.items);
        x.sync();
        synced = true;
        for (int i = 0; i < n; ++i) {
            bool in_range;
            run.fold(sb.at[i].first, sb.at[i].second, (size_t)fr[i].npoly * fr[i].ell, in_range);
            if (!in_range)
                throw Error(FHELIN_ERR_ARG, "import_device_many: frame " + std::to_string(i) + " holds a residue not below its modulus (range check)");
        }
    }
    hand_over(x, caller, synced);
    for (int i = 0; i < n; ++i) outs[i] = wrap(c, cts[i]);   // imported: not a level-plan source, never lowered
    FHELIN_CATCH
}

}  // extern "C"
