// read_out_trial.cpp -- TEST-ONLY: the address arithmetic of the wave kernels' output cursor and template source (rsq_reads.h: WaveReadOut, WaveFragmentSrc) on
// the CPU, beside the pointer forms they replace (WordColumn::at through RawLayout, FragmentSrc's words + word_off and sys_).  Addresses are formed from made-up
// array bases and compared as numbers; nothing at them is read or written, so pitches and positions of any size cost nothing.  The replay runs both cursors on real
// (small) arrays.  tests/test_read_out_offsets.py compiles this with g++.
#include <stdint.h>
#include <string.h>

#include <vector>

#include "../../reseq_amd/csrc/rsq_reads.h"

using namespace rsq;

extern "C" {

// made-up bases, far apart, 256-byte aligned like the allocator's
static uint32_t *const kSeq = reinterpret_cast<uint32_t *>(0x100000000000ull);
static const uint64_t *const kRefWords = reinterpret_cast<const uint64_t *>(0x200000000000ull);
static const uint64_t *const kTemplates = reinterpret_cast<const uint64_t *>(0x300000000000ull);
static const uint16_t *const kSysFwd = reinterpret_cast<const uint16_t *>(0x400000000000ull);
static const uint16_t *const kSysRev = reinterpret_cast<const uint16_t *>(0x500000000000ull);

int read_out_trial_wide(uint64_t words, uint64_t pitch) { return read_out_is_wide(words, pitch) ? 1 : 0; }

// word w of row `row` of an array of `words` word rows with `pitch` reads each: bytes from the array's base by the wave cursor (as the host sets `wide` for
// such arrays), out[0], and by WordColumn::at on RawLayout's column, out[1]
void read_out_trial_word(uint64_t words, uint64_t pitch, uint64_t row, uint32_t w, uint64_t *out) {
    RawLayout raw{};
    raw.seq = raw.qual = raw.ops = kSeq;
    raw.pitch = pitch;
    raw.wide = read_out_is_wide(words, pitch) ? 1u : 0u;
    const WaveReadOut wave = raw.wave_out_of(row);
    out[0] = (uint64_t)(reinterpret_cast<const char *>(wave.at(kSeq, w)) - reinterpret_cast<const char *>(kSeq));
    out[1] = (uint64_t)(reinterpret_cast<const char *>(&raw.seq_of(row).at(w)) - reinterpret_cast<const char *>(kSeq));
}

// A mate's template: its sequence begins at word `word_off` of the copy of the reference `hap_off` words behind the reference's own, its first systematic error is
// entry `sys_off` of the strand's track, and with `template_at` != ~0 its converted template begins at that word of the templates.  For template base k, as
// element indices from the arrays' bases: out[0] the word the wave source reads, out[1] the word FragmentSrc reads, out[2] / out[3] the same for the group of four
// errors, out[4] / out[5] which array each (0 reference, 1 templates; 0 forward track, 1 reverse track, in bit 1).
void read_out_trial_source(uint64_t word_off, uint64_t hap_off, uint64_t sys_off, int reverse, uint32_t first, uint64_t template_at, uint32_t k, uint64_t *out) {
    DevSim S{};
    S.ref_words = kRefWords;
    S.sys_fwd = kSysFwd;
    S.sys_rev = kSysRev;
    FragmentSrc src;
    src.words = kRefWords + hap_off;
    src.word_off = word_off;
    src.first = first;
    src.len = 0xFFFFu;
    src.reverse = reverse != 0;
    src.sys_ = (reverse ? kSysRev : kSysFwd) + sys_off;
    const bool converted = template_at != ~0ull;
    src.converted = converted ? kTemplates + template_at : nullptr;
    src.gc_prefix = nullptr;
    const WaveFragmentSrc wave = wave_fragment_src(S, src, converted ? kTemplates : nullptr, converted ? template_at : 0u);
    const uint64_t *base_w = converted ? kTemplates : kRefWords;
    const uint16_t *base_s = reverse ? kSysRev : kSysFwd;
    // the positions as base() of both sources takes them
    const uint32_t pos_wave = (wave.bits & WaveSrcBits::kBackward) ? wave.first - 1u - k : wave.first + k;
    const uint32_t pos_old = converted ? k : (src.reverse ? src.first - 1u - k : src.first + k);
    out[0] = (uint64_t)(wave.word_at(pos_wave >> 5) - base_w);
    out[1] = (uint64_t)((converted ? src.converted : src.words + src.word_off) + (pos_old >> 5) - base_w);
    out[2] = (uint64_t)(wave.sys_at(k & ~3u) - base_s);
    out[3] = (uint64_t)(src.sys_ + (k & ~3u) - base_s);
    out[4] = (wave.words == kTemplates ? 1u : 0u) | (((wave.bits & WaveSrcBits::kRevStrand) ? 1u : 0u) << 1) | (((wave.bits & WaveSrcBits::kBackward) ? 1u : 0u) << 2);
    out[5] = (converted ? 1u : 0u) | ((src.reverse ? 1u : 0u) << 1) | ((!converted && src.reverse ? 1u : 0u) << 2);
}

// The same n iterations through ReadOut and through WaveReadOut into arrays of `pitch` reads, row `row`: kinds[i] = 0 a base with op 0, 1 a deletion (op 1, no
// base), 2 an insertion (a base, op 2), 3 a tail iteration (a base, no op; only behind all others).  Returns 0 when the three arrays come out equal, word for
// word, the untouched words included.
int read_out_trial_replay(const uint8_t *kinds, uint32_t n, uint32_t pitch, uint32_t row, int wide) {
    const uint32_t words = n / 4u + 2u, ops_words = n / 16u + 2u;
    std::vector<uint32_t> a_seq((size_t)words * pitch, 0xA5A5A5A5u), a_qual(a_seq), a_ops((size_t)ops_words * pitch, 0xA5A5A5A5u), b_seq(a_seq), b_qual(a_seq), b_ops(a_ops);
    RawLayout ra{}, rb{};
    ra.seq = a_seq.data(), ra.qual = a_qual.data(), ra.ops = a_ops.data(), ra.pitch = pitch;
    rb.seq = b_seq.data(), rb.qual = b_qual.data(), rb.ops = b_ops.data(), rb.pitch = pitch, rb.wide = wide ? 1u : 0u;
    ReadOut old = ra.out_of(row);
    WaveReadOut wave = rb.wave_out_of(row);
    uint32_t pos = 0, n_ops = 0;
    for (uint32_t it = 0; it < n; ++it) {
        const uint32_t kind = kinds[it], base = (it * 7u + 1u) % 5u, qual = 33u + it % 41u;
        if (kind != 1u) {
            old.put(pos, base, qual);
            wave.put(pos, base, qual);
            ++pos;
        }
        if (kind != 3u) {
            old.op(it, kind);
            wave.op(it, kind);
            ++n_ops;
        }
    }
    old.finish();
    wave.finish(pos, n_ops);
    return (a_seq == b_seq ? 0 : 1) | (a_qual == b_qual ? 0 : 2) | (a_ops == b_ops ? 0 : 4);
}
}
