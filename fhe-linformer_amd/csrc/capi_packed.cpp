// extern "C" boundary, part 12: packed ciphertext blobs (include/fhelin.h "Packed formats": the stream and the blob are documented
// there).  Export range-checks, digests and packs on the device and downloads only the packed words.  The header codec is
// wire_header.h (CP_FORMATS); widths, the pack table and the digest run are wire.h's; the import is wire.cpp's import_blobs: the packed
// words uploaded, every blob's vectors unpacked in one launch (kernels_pack.hip), then the range check and digest of the other loaders
// on the unpacked residues (kernels_keys.hip) and every seeded c1 expanded in one launch (kernels_seeded.hip).  One synchronisation per
// call.
#include "../../include/fhelin.h"
#include <hip/hip_runtime.h>
#include <vector>
#include "capi_internal.h"
#include "wire.h"

using namespace fhelin;

namespace {

const char* const NOT_SEEDED = "packed seeded form: only an unmodified seeded (secret-key) encryption has one";

// the debug entry points take the widths themselves: each checked, the packed words of all
size_t debug_words(const Context& x, const int32_t* widths, int n_vec, const char* who) {
    if (x.N % 4096) throw Error(FHELIN_ERR_ARG, std::string(who) + ": ring dimension below 2^12");
    size_t total = 0;
    for (int i = 0; i < n_vec; ++i) total += pack_words(x.N, check_pack_width(widths[i], who));
    return total;
}

}  // namespace

extern "C" {

int fhelin_ct_packed_bytes(fhelin_ctx* c, const fhelin_ct* ct, int32_t seeded, size_t* bytes) {
    if (!c || !ct || !bytes) return capi_fail(FHELIN_ERR_ARG, "null argument");
    FHELIN_TRY
    if (seeded) {
        if (!ct->p || !ct->p->seeded) throw Error(FHELIN_ERR_STATE, NOT_SEEDED);
    } else {
        force(c, ct);
        if (ct->p->wrapped()) throw Error(FHELIN_ERR_ARG, "packed full form: a wrapped input has the seeded form only");
        if (ct->p->npoly < 2 || ct->p->npoly > 3) throw Error(FHELIN_ERR_ARG, "packed full form: 2 or 3 components");
    }
    *bytes = blob_header_of(CP_FORMATS[0], c->ctx, *ct->p, seeded ? 1 : ct->p->npoly).bytes();
    FHELIN_CATCH
}

int fhelin_ct_export_packed(fhelin_ctx* c, const fhelin_ct* ct, int32_t seeded, uint8_t* out, size_t cap) {
    if (!c || !ct || !out) return capi_fail(FHELIN_ERR_ARG, "null argument");
    FHELIN_TRY
    if (seeded && (!ct->p || !ct->p->seeded)) throw Error(FHELIN_ERR_STATE, NOT_SEEDED);
    const bool wrapped = seeded && ct->p->wrapped();   // a wrapped input is not a value of the pass (no level-plan terminal)
    const CtPtr& p = wrapped ? ct->p : terminal_in(c, ct);   // a wrapped handle with seeded = 0: FHELIN_ERR_ARG from ct_in
    Context& x = c->ctx;
    x.require_device();
    if (x.N % 4096) throw Error(FHELIN_ERR_ARG, "export_packed: ring dimension below 2^12");
    if (!seeded && (p->npoly < 2 || p->npoly > 3)) throw Error(FHELIN_ERR_ARG, "export_packed: 2 or 3 components");
    BlobHeader h = blob_header_of(CP_FORMATS[0], x, *p, seeded ? 1 : p->npoly);
    if (cap < h.bytes()) throw Error(FHELIN_ERR_ARG, "export_packed: buffer too small");
    // range check + digest of the unpacked residues and the pack, one after the other on the stream; only packed words come back
    const size_t n_vec = (size_t)h.stored * h.ell, words = (size_t)h.stored * h.words_per_poly;
    Scratch<u64> packed = x.scratch<u64>(words);
    std::vector<PackEntry> tab;
    pack_rows(tab, x.N, p->d, n_vec, h.width.data(), h.ell, packed, false);
    Scratch<PackEntry> d_tab = upload_pack_table(x, tab);
    launch_pack_residues(d_tab, (int)n_vec, x.N, x.stream);
    hip_check(hipGetLastError(), "packed export kernels");
    DigestRun run(x, {DigestItem{p->d, n_vec, 0, h.ell, h.ell}});   // after the pack launch: its download is the first thing to wait
    hip_check(hipMemcpyAsync(out + h.header_bytes(), packed, words * 8, hipMemcpyDeviceToHost, x.stream), "packed export");
    hip_check(hipStreamSynchronize(x.stream), "packed export sync");
    bool in_range;
    h.digest = run.fold(0, 0, n_vec, in_range);
    if (!in_range) throw Error(FHELIN_ERR_INTERNAL, "export_packed: the ciphertext holds a residue out of range");
    write_blob_header(h, out);
    FHELIN_CATCH
}

int fhelin_packed_info(const uint8_t* blob, size_t bytes, int32_t* log_n, int32_t* ell, int32_t* deg, int32_t* slots, int32_t* stored,
                       int32_t* count) {
    FHELIN_TRY
    const BlobHeader h = read_blob_header(CP_FORMATS, 1, blob, bytes);
    if (log_n) *log_n = h.log_n;
    if (ell) *ell = h.ell;
    if (deg) *deg = h.deg;
    if (slots) *slots = h.slots;
    if (stored) *stored = h.stored;
    if (count) *count = h.count;
    FHELIN_CATCH
}

int fhelin_ct_import_packed(fhelin_ctx* c, const uint8_t* const* blobs, const size_t* sizes, int32_t n, fhelin_ct** outs) {
    if (!c || (n > 0 && (!blobs || !sizes || !outs)) || n < 0) return capi_fail(FHELIN_ERR_ARG, "null argument");
    FHELIN_TRY
    import_blobs(c, "import_packed", CP_FORMATS, 1, blobs, sizes, n, outs);
    FHELIN_CATCH
}

int fhelin_debug_pack(fhelin_ctx* c, const uint64_t* words, const int32_t* widths, int32_t n_vec, uint64_t* out, size_t cap_words,
                      size_t* n_words) {
    if (!c || !words || !widths || !out || !n_words || n_vec < 1) return capi_fail(FHELIN_ERR_ARG, "null argument");
    FHELIN_TRY
    Context& x = c->ctx;
    x.require_device();
    const size_t N = x.N, total = debug_words(x, widths, n_vec, "debug_pack");
    for (int i = 0; i < n_vec; ++i)
        for (size_t j = 0; j < N; ++j)
            if (words[(size_t)i * N + j] >> widths[i]) throw Error(FHELIN_ERR_ARG, "debug_pack: a value at or above 2^w");
    if (cap_words < total) throw Error(FHELIN_ERR_ARG, "debug_pack: buffer too small");
    Scratch<u64> src = x.scratch<u64>((size_t)n_vec * N);
    Scratch<u64> dst = x.scratch<u64>(total);
    std::vector<PackEntry> tab;
    pack_rows(tab, N, src, n_vec, widths, n_vec, dst, false);
    hip_check(hipMemcpyAsync(src, words, (size_t)n_vec * N * 8, hipMemcpyHostToDevice, x.stream), "debug_pack upload");
    Scratch<PackEntry> d_tab = upload_pack_table(x, tab);
    launch_pack_residues(d_tab, n_vec, x.N, x.stream);
    hip_check(hipGetLastError(), "pack kernel");
    hip_check(hipMemcpyAsync(out, dst, total * 8, hipMemcpyDeviceToHost, x.stream), "debug_pack download");
    hip_check(hipStreamSynchronize(x.stream), "debug_pack sync");
    *n_words = total;
    FHELIN_CATCH
}

int fhelin_debug_unpack(fhelin_ctx* c, const uint64_t* packed, size_t n_words, const int32_t* widths, int32_t n_vec, uint64_t* out) {
    if (!c || !packed || !widths || !out || n_vec < 1) return capi_fail(FHELIN_ERR_ARG, "null argument");
    FHELIN_TRY
    Context& x = c->ctx;
    x.require_device();
    const size_t N = x.N, total = debug_words(x, widths, n_vec, "debug_unpack");
    if (n_words != total) throw Error(FHELIN_ERR_ARG, "debug_unpack: the word count does not match the widths");
    Scratch<u64> src = x.scratch<u64>(total);
    Scratch<u64> dst = x.scratch<u64>((size_t)n_vec * N);
    std::vector<PackEntry> tab;
    pack_rows(tab, N, dst, n_vec, widths, n_vec, src, true);
    hip_check(hipMemcpyAsync(src, packed, total * 8, hipMemcpyHostToDevice, x.stream), "debug_unpack upload");
    Scratch<PackEntry> d_tab = upload_pack_table(x, tab);
    launch_unpack_residues(d_tab, n_vec, x.N, x.stream);
    hip_check(hipGetLastError(), "unpack kernel");
    hip_check(hipMemcpyAsync(out, dst, (size_t)n_vec * N * 8, hipMemcpyDeviceToHost, x.stream), "debug_unpack download");
    hip_check(hipStreamSynchronize(x.stream), "debug_unpack sync");
    FHELIN_CATCH
}

int fhelin_debug_pack_rate(fhelin_ctx* c, const int32_t* widths, int32_t n_vec, int32_t reps, float* ms) {
    if (!c || !widths || !ms || n_vec < 1 || reps < 1) return capi_fail(FHELIN_ERR_ARG, "null argument");
    FHELIN_TRY
    Context& x = c->ctx;
    x.require_device();
    const size_t N = x.N, words = (size_t)n_vec * N, total = debug_words(x, widths, n_vec, "debug_pack_rate");
    Scratch<u64> a = x.scratch<u64>(words);
    Scratch<u64> b = x.scratch<u64>(words);
    Scratch<u64> pk = x.scratch<u64>(total);
    std::vector<PackEntry> tab;   // [n_vec] a -> pk, then [n_vec] pk -> b
    pack_rows(tab, N, a, n_vec, widths, n_vec, pk, false);
    pack_rows(tab, N, b, n_vec, widths, n_vec, pk, true);
    Scratch<PackEntry> d_tab = upload_pack_table(x, tab);
    hip_check(hipMemsetAsync(a, 0x15, words * 8, x.stream), "debug_pack_rate fill");
    struct Events {   // destroyed on every way out
        std::vector<hipEvent_t> v;
        explicit Events(size_t n) : v(n, nullptr) {}
        ~Events() {
            for (hipEvent_t e : v)
                if (e) (void)hipEventDestroy(e);
        }
    } events(4 * (size_t)reps + 1);
    std::vector<hipEvent_t>& ev = events.v;
    for (auto& e : ev) hip_check(hipEventCreate(&e), "hipEventCreate");
    // one untimed round, then pack, copy, unpack, copy in turn: the copy moves the same unpacked bytes device to device
    for (int r = -1; r < reps; ++r) {
        const bool timed = r >= 0;
        if (r == 0) hip_check(hipEventRecord(ev[0], x.stream), "hipEventRecord");
        launch_pack_residues(d_tab, n_vec, x.N, x.stream);
        if (timed) hip_check(hipEventRecord(ev[4 * r + 1], x.stream), "hipEventRecord");
        hip_check(hipMemcpyAsync(b, a, words * 8, hipMemcpyDeviceToDevice, x.stream), "debug_pack_rate copy");
        if (timed) hip_check(hipEventRecord(ev[4 * r + 2], x.stream), "hipEventRecord");
        launch_unpack_residues(d_tab + n_vec, n_vec, x.N, x.stream);
        if (timed) hip_check(hipEventRecord(ev[4 * r + 3], x.stream), "hipEventRecord");
        hip_check(hipMemcpyAsync(a, b, words * 8, hipMemcpyDeviceToDevice, x.stream), "debug_pack_rate copy");
        if (timed) hip_check(hipEventRecord(ev[4 * r + 4], x.stream), "hipEventRecord");
    }
    hip_check(hipGetLastError(), "pack kernels");
    hip_check(hipStreamSynchronize(x.stream), "debug_pack_rate sync");
    for (int k = 0; k < 4 * reps; ++k) hip_check(hipEventElapsedTime(&ms[k], ev[k], ev[k + 1]), "hipEventElapsedTime");
    FHELIN_CATCH
}

}  // extern "C"
