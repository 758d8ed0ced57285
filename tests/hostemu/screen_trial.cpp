// screen_trial.cpp -- TEST-ONLY: the read kernel's screened draw (rsq_core.h draw_screened, single precision with its error bound) beside the
// double-precision recipe (draw_rows_k, the reference's LogArrayResult::Draw) on rows the caller gives, on the CPU.  tests/test_screened_draw_bound.py
// compiles it (g++, -ffp-contract=off as the product) and checks that every draw the screen calls decided has the double-precision column.
#include <stdint.h>

#include <vector>

#include "../../reseq_amd/csrc/rsq_core.h"

using namespace rsq;

namespace {

template <int Q>
void trial(int nm, uint32_t k, const double *rows, uint32_t n, const uint32_t *words, int32_t *out) {
    const uint32_t kp = row_stride(k), slot = 4u * Q;
    std::vector<float> f32(4u * slot, 0.f);                  // the float copies as pack_tables writes them: four columns per quad, pad columns zero
    for (int m = 0; m < nm; ++m)
        for (uint32_t c = 0; c < k; ++c) f32[m * slot + c] = (float)rows[m * kp + c];
    const GlobalRow g0{rows}, g1{rows + kp}, g2{rows + 2u * kp}, g3{rows + 3u * kp};
    const GlobalRow32 h0{f32.data()}, h1{f32.data() + slot}, h2{f32.data() + 2u * slot}, h3{f32.data() + 3u * slot};
    for (uint32_t i = 0; i < n; ++i) {
        double ps;
        uint32_t col = 0, exact;
        bool decided;
        if (nm == 3) {
            decided = draw_screened<Q>(words[i], col, h0, h1, h2);
            exact = draw_rows_k(k, u32_to_unit(words[i]), ps, g0, g1, g2);
        } else {
            decided = draw_screened<Q>(words[i], col, h0, h1, h2, h3);
            exact = draw_rows_k(k, u32_to_unit(words[i]), ps, g0, g1, g2, g3);
        }
        out[3 * i] = decided;
        out[3 * i + 1] = (int32_t)col;
        out[3 * i + 2] = (int32_t)exact;
    }
}

}  // namespace

extern "C" {
// rows: nm (3 or 4) margins of row_stride(k) doubles each, zero past column k; k <= 48.  out: n x (decided, screened column, double-precision column)
int screen_trial(int nm, uint32_t k, const double *rows, uint32_t n, const uint32_t *words, int32_t *out) {
    if ((nm != 3 && nm != 4) || k < 1 || k > 48) return -1;
    switch ((k + 3u) / 4u) {
#define RSQ_TRIAL_CASE(q) \
    case q: trial<q>(nm, k, rows, n, words, out); return 0;
        RSQ_TRIAL_CASE(1) RSQ_TRIAL_CASE(2) RSQ_TRIAL_CASE(3) RSQ_TRIAL_CASE(4) RSQ_TRIAL_CASE(5) RSQ_TRIAL_CASE(6)
        RSQ_TRIAL_CASE(7) RSQ_TRIAL_CASE(8) RSQ_TRIAL_CASE(9) RSQ_TRIAL_CASE(10) RSQ_TRIAL_CASE(11) RSQ_TRIAL_CASE(12)
#undef RSQ_TRIAL_CASE
    }
    return -1;
}
// row_stride(k): the double rows' stride
uint32_t screen_row_stride(uint32_t k) { return row_stride(k); }
}
