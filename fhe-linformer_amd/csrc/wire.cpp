// Wire formats, device part (wire.h).
#include "wire.h"
#include <hip/hip_runtime.h>
#include <algorithm>
#include <map>
#include "kernels_keys.h"
#include "kernels_seeded.h"

namespace fhelin {

size_t pack_rows(std::vector<PackEntry>& tab, size_t N, u64* block, size_t rows, const int* width, int limbs, u64* packed, bool unpack) {
    size_t at = 0;
    for (size_t r = 0; r < rows; ++r) {
        const int w = width[r % (size_t)limbs];
        u64* row = block + r * N;
        tab.push_back(unpack ? PackEntry{packed + at, row, (u32)w, 0} : PackEntry{row, packed + at, (u32)w, 0});
        at += pack_words(N, w);
    }
    return at;
}

Scratch<PackEntry> upload_pack_table(Context& x, const std::vector<PackEntry>& tab) {
    static_assert(sizeof(PackEntry) == 24, "a table entry is three words");
    Scratch<PackEntry> d_tab = x.scratch<PackEntry>(tab.size());
    const size_t per = x.stage_words / 3;   // entries per piece
    for (size_t lo = 0; lo < tab.size(); lo += per) {
        const size_t cnt = std::min(per, tab.size() - lo);
        x.upload_async(reinterpret_cast<u64*>(d_tab + lo), reinterpret_cast<const u64*>(tab.data() + lo), 3 * cnt);
    }
    return d_tab;
}

DigestRun::DigestRun(Context& x, const std::vector<DigestItem>& items) {
    const size_t N = x.N;
    auto groups_per_launch = [](const DigestItem& it) { return std::max<size_t>(1, 65535 / (size_t)it.limb_count); };
    size_t total = 0, most = 0;
    for (const DigestItem& it : items) {
        at_.push_back(total);
        total += it.n_vec;
        most = std::max(most, std::min(it.n_vec, groups_per_launch(it) * it.limb_count));
    }
    if (!total) return;
    part_ = x.scratch<u64>(key_digest_scratch_words(x.N, (int)most));
    dg_ = x.scratch<u64>(2 * total);
    for (size_t k = 0; k < items.size(); ++k) {
        const DigestItem& it = items[k];
        const size_t step = groups_per_launch(it) * it.limb_count;   // whole groups: a launch starts at a group's first vector
        for (size_t v = 0; v < it.n_vec; v += step)
            launch_key_digest_strided(x.dt, it.d + v / it.limb_count * it.group_stride * N, (int)std::min(step, it.n_vec - v), it.limb_first,
                                      it.limb_count, it.group_stride, part_, dg_ + 2 * (at_[k] + v), x.stream);
    }
    hip_check(hipGetLastError(), "range check and digest kernels");
    h_.resize(2 * total);
    hip_check(hipMemcpyAsync(h_.data(), dg_, h_.size() * 8, hipMemcpyDeviceToHost, x.stream), "digest download");
}

ShapeBatch::ShapeBatch(fhelin_ctx* c, const std::vector<std::pair<int, int>>& shape) : cts(shape.size()), at(shape.size()) {
    std::map<std::pair<int, int>, std::vector<int>> groups;
    for (size_t i = 0; i < shape.size(); ++i) groups[shape[i]].push_back((int)i);
    for (auto& g : groups) {
        const int stored = g.first.first, ell = g.first.second;
        const size_t per = (size_t)stored * ell;
        std::vector<CtPtr> b = c->ev.new_ct_batch((int)g.second.size(), std::max(2, stored), ell, 1, 1.0L, 1);
        for (size_t k = 0; k < g.second.size(); ++k) {
            cts[g.second[k]] = b[k];
            at[g.second[k]] = {items.size(), k * per};
        }
        // the batch is one block [cnt][npoly][ell][N]: the stored vectors of a seeded form are ell apart in groups of 2 ell
        items.push_back(DigestItem{b[0]->d, g.second.size() * per, 0, ell, stored == 1 ? 2 * ell : ell});
        max_ell = std::max(max_ell, ell);
    }
}

BlobHeader blob_header_of(const BlobFormat& f, const Context& x, const Ciphertext& ct, int stored) {
    BlobHeader h;
    h.fmt = &f;
    h.log_n = x.prm.log_n;
    h.ell = ct.ell;
    h.deg = ct.deg;
    h.slots = ct.slots;
    h.set_scale(ct.scale);
    h.stored = stored;
    if (stored == 1) {
        h.nonce = ct.nonce;
        std::memcpy(h.seed, ct.seed, 32);
        if (ct.wrapped()) {
            h.count = (int32_t)ct.wrap_pos.size();
            h.total = ct.wrap_total;
            h.pos = ct.wrap_pos;
        }
    }
    // the first ell moduli of Q then P: for ell <= n_q that is chain.q[0..ell), since Context builds `moduli` as chain.q then chain.p
    h.moduli.assign(x.moduli.begin(), x.moduli.begin() + ct.ell);
    h.words_per_poly = blob_words_per_poly(f, h.log_n, h.moduli.data(), h.ell, &h.width);
    return h;
}

void import_blobs(fhelin_ctx* c, const std::string& who, const BlobFormat* fmts, size_t n_fmts, const uint8_t* const* blobs,
                  const size_t* sizes, int n, fhelin_ct** outs) {
    Context& x = c->ctx;
    x.require_device();
    if (n == 0) return;
    if (n > 65535) throw Error(FHELIN_ERR_ARG, who + ": at most 65535 blobs per call");
    if (x.N % 4096) throw Error(FHELIN_ERR_ARG, who + ": ring dimension below 2^12");
    const size_t N = x.N;
    auto blob = [&](int i) { return who + ": blob " + std::to_string(i); };
    // 1. every header, against the blob and against this context, before anything is allocated
    std::vector<BlobHeader> hs(n);
    std::vector<std::pair<int, int>> shape(n);
    size_t total_words = 0;
    for (int i = 0; i < n; ++i) {
        hs[i] = read_blob_header(fmts, n_fmts, blobs[i], sizes[i]);
        const BlobHeader& h = hs[i];
        if (h.log_n != x.prm.log_n) throw Error(FHELIN_ERR_ARG, blob(i) + ": made for another ring dimension");
        // wrapped: ell <= n_q + 1, the first ell moduli of Q then P (the extra limb of an input at n_q limbs is p_0)
        if (h.ell > x.L + 1 + (h.wrapped() && x.K > 0 ? 1 : 0)) throw Error(FHELIN_ERR_ARG, blob(i) + ": more limbs than the context's chain");
        if (std::memcmp(h.moduli.data(), x.moduli.data(), 8 * (size_t)h.ell) != 0) throw Error(FHELIN_ERR_ARG, blob(i) + ": moduli do not match the context");
        shape[i] = {h.stored, h.ell};
        total_words += (size_t)h.stored * h.words_per_poly;
    }
    // 2. one batch allocation per shape; a 64-bit payload is uploaded straight into its ciphertext, the packed payloads into one
    // scratch block that one launch unpacks
    ShapeBatch sb(c, shape);
    for (const DigestItem& it : sb.items)   // the run below would split such a shape between launches: refused as it always was
        if (it.n_vec > 65535) throw Error(FHELIN_ERR_ARG, who + ": too many limbs of one level in one call");
    const bool packed = fmts[0].packed;
    Scratch<u64> pk;
    if (packed) pk = x.scratch<u64>(total_words);
    std::vector<PackEntry> ptab;
    std::vector<SeededEntry> stab;
    size_t at = 0;
    for (int i = 0; i < n; ++i) {
        const BlobHeader& h = hs[i];
        Ciphertext& ct = *sb.cts[i];
        ct.deg = h.deg;
        ct.slots = h.slots;
        ct.scale = h.scale();
        if (h.wrapped()) {
            ct.wrap_pos = h.pos;
            ct.wrap_total = h.total;
        }
        const size_t words = (size_t)h.stored * h.words_per_poly;
        hip_check(hipMemcpyAsync(packed ? pk + at : ct.d, h.payload, words * 8, hipMemcpyHostToDevice, x.stream), "blob upload");
        if (packed) at += pack_rows(ptab, N, ct.d, (size_t)h.stored * h.ell, h.width.data(), h.ell, pk + at, true);
        if (h.stored == 1) {   // c1 is the expansion of the public (seed, nonce)
            SeededEntry e;
            for (int w = 0; w < 8; ++w) e.key.w[w] = get<uint32_t>(h.seed, 4 * w);
            e.nonce = h.nonce;
            e.dst = ct.d + (size_t)h.ell * N;
            e.ell = h.ell;
            stab.push_back(e);
        }
    }
    // 3. unpack everything in one launch; range check + digest of the 64-bit residues; every seeded c1 in one launch; one
    // synchronisation for the call (not a Context::sync: the blob paths are outside its count)
    Scratch<PackEntry> d_ptab;
    if (packed) {
        d_ptab = upload_pack_table(x, ptab);
        launch_unpack_residues(d_ptab, (int)ptab.size(), x.N, x.stream);
    }
    Scratch<SeededEntry> d_stab;
    if (!stab.empty()) {
        d_stab = x.scratch<SeededEntry>(stab.size());
        hip_check(hipMemcpyAsync(d_stab, stab.data(), stab.size() * sizeof(SeededEntry), hipMemcpyHostToDevice, x.stream), "seed table upload");
        launch_seeded_expand(x.dt, d_stab, (int)stab.size(), sb.max_ell, x.stream);
    }
    DigestRun run(x, sb.items);
    hip_check(hipStreamSynchronize(x.stream), "blob import sync");
    // 4. all or nothing: a handle only when every blob passed
    for (int i = 0; i < n; ++i) {
        bool in_range;
        const u64 digest = run.fold(sb.at[i].first, sb.at[i].second, (size_t)hs[i].stored * hs[i].ell, in_range);
        if (!in_range) throw Error(FHELIN_ERR_ARG, blob(i) + " holds a residue not below its modulus (range check)");
        if (digest != hs[i].digest) throw Error(FHELIN_ERR_ARG, blob(i) + " does not match its digest");
    }
    for (int i = 0; i < n; ++i) outs[i] = wrap(c, sb.cts[i]);   // imported: not a level-plan source, never lowered
}

}  // namespace fhelin
