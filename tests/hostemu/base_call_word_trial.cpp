// base_call_word_trial.cpp -- TEST-ONLY: the base call decided by the random word alone (rsq_pack.h base_call_word_bounds, rsq_reads.h word_screen_sure and
// ScreenTables::base_call_word), built by tests/test_base_call_word.py on top of the host emulation (this file includes hostemu.cpp: the same emu_* entry points,
// and the emulation's own structures for the functions below).
//  * bcw_share: the reads of a list of fragments in the read kernel's grouping -- 64 consecutive pairs of one template segment are a wave, and the wave's step t is
//    iteration t of each of its reads -- with, per base-call draw, whether the word decided it: the share of such lanes and of wave-steps in which every
//    drawing lane is decided (only those skip the draw's branch).
//  * bcw_soundness: one made-up table through the pack-time bound; every word the check calls sure, for every combination of list entries and every combination
//    of values that share those entries, is drawn in double precision (draw<4>: LogArrayResult::Draw) and must give the template base, or prob_sum 0.
#include <stdint.h>
static int g_bcw_last = -1;
#define RSQ_WORD_SCREEN_STATS(sure) (g_bcw_last = (sure) ? 1 : 0)
#include "hostemu.cpp"

namespace {

// one read as run_read runs it (ring lag 0), with the outcome of the word screen per iteration: -1 no base-call draw, 0 not sure, 1 sure
template <uint32_t M>
void traced_read(Emu &s, uint32_t seg, const Stream &st, uint32_t tile, uint32_t frag_len, const FragmentSrc &src, std::vector<int8_t> &trace) {
    Raw raw;
    ReadOut out = raw.out(s);
    float *img = s.image(seg, tile), *ring = img + s.dev.lds.ring_off;
    const uint32_t qbase = image_qbase(s.dev, seg, s.dev.lds.binned ? tile : 0u);
    ScreenTables<M> tab{s.dev, img, qbase, ring, 0u};
    ReadMachine m;
    m.init(s.dev, tab, st, seg, tile, frag_len, src);
    for (;;) {
        const uint32_t t = m.par.read_pos;
        for (uint32_t item = 0; item < lds_ring_items(s.dev); ++item) {
            const RingItem it = lds_ring_item(s.dev, qbase, item);
            for (uint32_t back = 0; back <= kRingLag && back <= t; ++back) lds_ring_stage(s.dev, it, ring, t - back);
        }
        tab.t = t;
        g_bcw_last = -1;
        if (m.in_template()) m.template iterate<true>(s.dev, tab, st, src, out);
        else if (!m.step(s.dev, tab, st, src, out)) break;
        trace.push_back((int8_t)g_bcw_last);
    }
}

}  // namespace

extern "C" {

// out[4]: base-call draws, those the word decided, wave-steps with a base-call draw, those in which the word decided every one
int bcw_share(void *h, const Fragment *frags, uint64_t n_pairs, uint64_t *out) {
    Emu &s = *static_cast<Emu *>(h);
    return guard([&] {
        if (s.has_variants || s.dev.meth_ptr || !s.mask()) throw Error("bcw_share: plain pairs on the screened route only");
        out[0] = out[1] = out[2] = out[3] = 0;
        for (uint32_t seg = 0; seg < 2; ++seg)
            for (uint64_t first = 0; first < n_pairs; first += 64) {
                std::vector<std::vector<int8_t>> lanes;
                for (uint64_t pair = first; pair < std::min<uint64_t>(first + 64, n_pairs); ++pair) {
                    const Fragment &f = frags[pair];
                    const uint32_t c2 = f.len | ((uint32_t)f.dup << 16), c1 = f.seq;
                    const Stream st{s.dev.seed, f.start, c1, c2, pair_c3(kDomPair, f.strand, seg, f.allele)};
                    const uint32_t tile = draw_tile(s.dev, f.start, c1, c2, pair_c3(kDomPair, f.strand, 2, f.allele));
                    const FragmentSrc src = fragment_src(s.dev, f, seg);
                    lanes.emplace_back();
                    bool done = false;
                    auto run = [&](auto tag) {
                        constexpr uint32_t M = decltype(tag)::value;
                        if (s.mask() != M) return;
                        traced_read<M>(s, seg, st, tile, f.len, src, lanes.back());
                        done = true;
                    };
                    run(std::integral_constant<uint32_t, kQualityQuads[0]>{});
                    run(std::integral_constant<uint32_t, kQualityQuads[1]>{});
                    run(std::integral_constant<uint32_t, kQualityQuads[2]>{});
                    run(std::integral_constant<uint32_t, kQualityQuads[3]>{});
                    run(std::integral_constant<uint32_t, kQualityQuads[4]>{});
                    if (!done) throw Error("no screened instantiation for the plan's mask");
                }
                size_t steps = 0;
                for (const auto &l : lanes) steps = std::max(steps, l.size());
                for (size_t t = 0; t < steps; ++t) {
                    uint32_t draws = 0, sure = 0;
                    for (const auto &l : lanes)
                        if (t < l.size() && l[t] >= 0) ++draws, sure += (uint32_t)l[t];
                    out[0] += draws;
                    out[1] += sure;
                    out[2] += draws ? 1u : 0u;
                    out[3] += draws && sure == draws ? 1u : 0u;
                }
            }
    });
}

// whether the LDS plan of the simulator has the word screen's scalars, and how they are laid out: out[0] staged, [1] words per table, [2..5] caps, [6] the sides checked
void bcw_plan(void *h, uint32_t *out) {
    const LdsPlan &p = static_cast<Emu *>(h)->dev.lds;
    out[0] = p.bw_off != kNoLds;
    out[1] = p.bw_stride;
    for (int n = 0; n < 4; ++n) out[2 + n] = p.bw_cap[n];
    out[6] = p.bw_sides;
}

// One table of k columns with outcome values par0[k], margin n over values from[n] .. from[n] + rows[n] - 1 (values: the margins' rows one after the other, k doubles
// each), in a family whose common ranges are g_from / g_last; `base` the template base; every stored scalar is multiplied by `cut` (1: as packed; below 1: the
// negative control).  out[0] the table has a bound, [1] (entries, word) pairs found sure, [2] draws checked, [3] draws that did not give the template base,
// [4] draws with prob_sum 0 among the checked.
int bcw_soundness(uint32_t k, const uint8_t *par0, const uint32_t *from, const uint32_t *rows, const double *values, const uint32_t *g_from, const uint32_t *g_last, uint32_t base, double cut,
                  uint64_t *out) {
    return guard([&] {
        DevTable d{};
        d.k = k;
        d.f32_ok = 1;
        const uint32_t kp = row_stride(k);
        std::vector<double> pool;
        const double *v = values;
        for (uint32_t n = 0; n < 4; ++n) {
            d.from[n] = from[n];
            d.rows[n] = rows[n];
            d.off[n] = (uint32_t)pool.size();
            for (uint32_t r = 0; r < rows[n]; ++r, v += k) {
                for (uint32_t c = 0; c < kp; ++c) pool.push_back(c < k ? v[c] : 0.0);
                for (uint32_t c = 0; c < k; ++c)
                    if (!(v[c] == 0.0 || (v[c] >= 0x1p-60 && v[c] <= 0x1p29))) d.f32_ok = 0;      // as pack_tables decides it
            }
        }
        pool.resize(pool.size() + 16, 0.0);
        FamilyGeo g{};
        for (uint32_t n = 0; n < 4; ++n) g.from[n] = g_from[n], g.last[n] = g_last[n];
        const WordScreenGeo w = word_screen_geo(g);
        std::vector<float> lists(2u * w.stride);
        uint32_t sides = 0;
        out[0] = base_call_word_bounds(d, pool.data(), par0, base, g, w, lists.data(), &sides) ? 1u : 0u;
        out[1] = out[2] = out[3] = out[4] = 0;
        if (!sides) sides = 1u;                                    // as pack_tables
        for (float &x : lists) x = (float)(x * cut);
        const Float2 *pairs = reinterpret_cast<const Float2 *>(lists.data());
        uint32_t e[4];
        auto values_of = [&](uint32_t n, uint32_t entry, uint32_t &lo, uint32_t &hi) {       // the values a lane with this entry may hold
            const uint32_t sh = 1 == n ? kWordPosShift : 0u;
            lo = entry << sh;
            hi = entry < w.cap[n] ? ((entry + 1u) << sh) - 1u : std::max(lo, g.from[n] + g.last[n]) + 2u;      // and beyond the common range
        };
        for (e[0] = 0; e[0] <= w.cap[0]; ++e[0])
            for (e[1] = 0; e[1] <= w.cap[1]; ++e[1])
                for (e[2] = 0; e[2] <= w.cap[2]; ++e[2])
                    for (e[3] = 0; e[3] <= w.cap[3]; ++e[3]) {
                        const Float2 a = pairs[e[0]], p = pairs[w.at[1] + e[1]], q = pairs[w.at[2] + e[2]], r = pairs[w.at[3] + e[3]];
                        auto sure = [&](uint64_t word) { return word <= 0xFFFFFFFFull && word_screen_sure(a, p, q, r, (uint32_t)word, sides); };
                        // the sure words are one range (the check's two sums are monotone in the word): its ends by bisection from a sure word
                        uint64_t inside = 0x100000000ull;
                        for (uint64_t probe : {0ull, 1ull, 0x40000000ull, 0x80000000ull, 0xC0000000ull, 0xFFFFFFFFull})
                            if (sure(probe)) inside = probe;
                        if (inside > 0xFFFFFFFFull) continue;
                        uint64_t lo_out = 0, lo_in = inside, hi_in = inside, hi_out = 0x100000000ull;      // first sure word in (lo_out, lo_in], last in [hi_in, hi_out)
                        const bool from_zero = sure(0);
                        while (!from_zero && lo_in - lo_out > 1) {
                            const uint64_t mid = (lo_in + lo_out) / 2;
                            (sure(mid) ? lo_in : lo_out) = mid;
                        }
                        if (from_zero) lo_in = 0;
                        while (hi_out - hi_in > 1) {
                            const uint64_t mid = (hi_in + hi_out) / 2;
                            (sure(mid) ? hi_in : hi_out) = mid;
                        }
                        std::vector<uint64_t> words;
                        for (uint64_t end : {lo_in, hi_in})
                            for (int64_t off : {-2, -1, 0, 1, 2, 65536, -65536}) words.push_back(end + (uint64_t)off);
                        words.push_back((lo_in + hi_in) / 2);
                        for (uint64_t word : words) {
                            if (!sure(word)) continue;
                            ++out[1];
                            uint32_t lo[4], hi[4], idx[4];
                            for (uint32_t n = 0; n < 4; ++n) values_of(n, e[n], lo[n], hi[n]);
                            for (idx[0] = lo[0]; idx[0] <= hi[0]; ++idx[0])
                                for (idx[1] = lo[1]; idx[1] <= hi[1]; ++idx[1])
                                    for (idx[2] = lo[2]; idx[2] <= hi[2]; ++idx[2])
                                        for (idx[3] = lo[3]; idx[3] <= hi[3]; ++idx[3]) {
                                            double ps;
                                            const uint32_t value = draw<4>(d, pool.data(), par0, idx, u32_to_unit((uint32_t)word), ps);
                                            ++out[2];
                                            if (0.0 == ps) ++out[4];
                                            else if (value != base) ++out[3];
                                        }
                        }
                    }
    });
}

}  // extern "C"
