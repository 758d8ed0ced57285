// rsq_prepass.h -- the host side of the pre-passes, once (host only): the plan, the bias normalisation, the systematic-error chains, the sharded variants of these
// (rsq_sim_prepare_plan ... rsq_sim_prepare_finish) and the systematic-error profile.  What runs between the calls -- their order, which run of the chains is reused
// or resumed, the states that cross a shard's borders -- is written here against PrepassSim (SimState and what the pre-passes keep), the Uploader and a PrepassBackend.  The backend is what
// differs between the library (rsq_sim.hip: kernels and device arrays) and the host emulation of the tests (tests/hostemu/hostemu.cpp: loops over the lanes' functions).
#pragma once
#include <chrono>

#include "rsq_pack.h"

namespace rsq {

// a run of the systematic-error chains: the host's part (the chunks' states live with the backend that runs the passes)
struct ChainRun {
    std::vector<Chain> chains;
    ShardEdges edges;
    uint32_t n_chunks = 0, passes = 0, block_lo = 0, block_hi = 0;
    bool pass_through = false;     // the rank has no blocks: its neighbours' states go straight through
    bool valid = false;
};
// the simulator's state and, in one place, what the pre-passes keep between their calls: both simulators (rsq_sim, the emulation's) are one of these
struct PrepassSim : SimState {
    struct {
        BiasPlan bias_plan;        // the sharded pre-pass (rsq_sim_prepare_plan ... rsq_sim_prepare_finish)
        bool planned = false;      // rsq_sim_prepare_plan has run, and no rsq_sim_prepare since
        bool normalized = false;   // rsq_sim_prepare_normalization has run since the plan
        ChainRun run;              // the last run of the chains
    } pre;
};

struct PrepassBackend {
    // partial sums and maxima of the chunks (kBiasBlock * kBiasRun start positions each, BiasPlan::chunk_ptr) whose first start position lies in the share
    // [g_lo, g_hi) of the concatenated sequences, g_lo < g_hi; sums / maxes: bias_chunks(plan) zeros, the other chunks stay zero
    virtual void bias_partials(const BiasPlan &plan, uint64_t g_lo, uint64_t g_hi, std::vector<double> &sums, std::vector<double> &maxes) = 0;
    // a new run: room for the states of its n_chunks > 0 chunks (entering state used, outgoing states of two passes); chunk_chain: the chain of every chunk
    virtual void begin_run(const ChainRun &run, const std::vector<uint32_t> &chunk_chain) = 0;
    virtual void publish_chains(const ChainRun &run) = 0;                      // run.chains has changed (Chain::in_state)
    // one pass: every chunk in pass 0, later the chunks whose incoming state (the left neighbour's in out[prev]) differs from the one they used; the others' outgoing
    // states are carried from out[prev] to out[cur].  Returns how many chunks ran.
    virtual uint32_t run_pass(const ChainRun &run, uint32_t pass, int prev, int cur) = 0;
    virtual uint32_t out_state(const ChainRun &run, int cur, size_t chunk) = 0;       // the outgoing state of one chunk
    virtual void variant_sys_errors(const ChainRun &run) = 0;                  // -V: the variants' own systematic errors, from the finished run
    virtual void ready_to_simulate() = 0;                                      // what is made once per pre-pass for the read kernels
    virtual ~PrepassBackend() {}
};

// dom | rate << 8 per position, as the chains write their tracks -> the two byte arrays of the ABI and of the profile's FASTQ records
inline void read_sys_track(Uploader &up, const uint16_t *track, uint32_t len, uint8_t *dom, uint8_t *rate) {
    std::vector<uint16_t> tmp(len);
    up.read_bytes(tmp.data(), track, (size_t)len * 2);
    for (uint32_t i = 0; i < len; ++i) {
        dom[i] = (uint8_t)(tmp[i] & 0xFF);
        rate[i] = (uint8_t)(tmp[i] >> 8);
    }
}

// ------------------------------------------------------------------------------- systematic errors (a13)
// passes over the run's chunks until no chunk's incoming state changed; `first_pass`: 0 for a new run, the run's pass count to resume one whose
// entering states (Chain::in_state) were replaced: only the chunks behind a changed state run again
inline void iterate_chains(ChainRun &run, PrepassBackend &be, uint32_t first_pass) {
    uint32_t pass = first_pass;
    for (;; ++pass) {
        const uint32_t n_run = be.run_pass(run, pass, (pass + 1) & 1, pass & 1);
        if (pass > 0 && !n_run) break;
        if (pass > first_pass + run.n_chunks + 2) throw Error("systematic-error chains did not converge");
    }
    run.passes = pass + 1;                                          // the final states are in out[(run.passes - 1) & 1]
}
inline uint32_t run_chains(PrepassSim &s, PrepassBackend &be, ChainSet set, const ShardRange *range = nullptr) {
    ChainRun &run = s.pre.run;
    run.valid = false;
    run.chains.clear();
    run.edges = ShardEdges{};
    std::vector<uint32_t> chunk_chain;
    s.chain_chunk = chain_chunk_len(s.total_ref_size, s.opt);
    build_chains(s, set, run.chains, chunk_chain, range, &run.edges);
    run.n_chunks = (uint32_t)chunk_chain.size();
    run.passes = 0;
    if (!run.n_chunks) return 0;
    be.begin_run(run, chunk_chain);
    iterate_chains(run, be, 0);
    run.valid = true;
    return run.passes;
}

// ------------------------------------------------------------------------------- bias normalisation (a14)
inline void share_bias_partials(PrepassBackend &be, const BiasPlan &plan, uint64_t g_lo, uint64_t g_hi, std::vector<double> &sums, std::vector<double> &maxes) {
    sums.assign(bias_chunks(plan), 0.0);
    maxes.assign(sums.size(), 0.0);
    if (g_lo < g_hi) be.bias_partials(plan, g_lo, g_hi, sums, maxes);      // a rank without blocks adds nothing
}

// ------------------------------------------------------------------------------- the whole pre-pass (rsq_sim_prepare)
inline void prepare(PrepassSim &s, Uploader &up, PrepassBackend &be, uint64_t seed, uint64_t num_read_pairs, double coverage, int ref_bias_mode, const char *base_identifier) {
    const bool trace = s.opt.trace_prepare != 0;                // stage times of the pre-pass on stderr
    auto now = [] { return std::chrono::steady_clock::now(); };
    auto lap = [&](const char *what, std::chrono::steady_clock::time_point &t0) {
        if (trace) fprintf(stderr, "prepare: %-28s %8.3f s\n", what, std::chrono::duration<double>(now() - t0).count());
        t0 = now();
    };
    auto t0 = now();
    plan_simulation(s, up, seed, num_read_pairs, coverage, ref_bias_mode, base_identifier);
    lap("plan", t0);
    s.pre.planned = false;
    if (s.has_ref) {
        const BiasPlan plan = plan_bias_normalization(s, up);
        std::vector<double> sums, maxes;
        share_bias_partials(be, plan, 0, UINT64_MAX, sums, maxes);
        normalization_from_partials(s, up, plan, sums.data(), maxes.data());
        lap("bias normalisation", t0);
    }
    s.passes = run_chains(s, be, s.has_ref ? kChainsSimulation : kChainsAdapters);      // every pass but the first ends by waiting for its count: nothing is in flight here
    lap("systematic-error chains", t0);
    if (s.has_variants && s.pre.run.valid) be.variant_sys_errors(s.pre.run);      // -V: the variants' bases, from the finished chains
    lap("variants' systematic errors", t0);
    s.prepared = true;
    s.prepared_lo = 1;
    s.prepared_hi = s.total_blocks + 1;
    be.ready_to_simulate();
    lap("read kernel for the profile", t0);
}

// ------------------------------------------------------------------------------- the sharded pre-pass (rsq_sim_prepare_plan ... rsq_sim_prepare_finish)
inline void require_plan(const PrepassSim &s) {
    if (!s.pre.planned) throw Error("rsq_sim_prepare_plan must run first");
}
inline void prepare_plan(PrepassSim &s, Uploader &up, uint64_t seed, uint64_t num_read_pairs, double coverage, int ref_bias_mode, const char *base_identifier) {
    if (!s.has_ref) throw Error("the sharded pre-pass needs a reference");
    s.prepared = false;
    s.pre.normalized = false;
    s.pre.run.valid = false;
    plan_simulation(s, up, seed, num_read_pairs, coverage, ref_bias_mode, base_identifier);
    s.pre.bias_plan = plan_bias_normalization(s, up);
    s.pre.planned = true;
}
// sums / maxes: bias_chunks(s.pre.bias_plan) values each
inline void prepare_bias_partials(PrepassSim &s, PrepassBackend &be, uint32_t block_lo, uint32_t block_hi, double *sums, double *maxes) {
    require_plan(s);
    const ShardRange r = shard_range(s, block_lo, block_hi);
    std::vector<double> h_sum, h_max;
    share_bias_partials(be, s.pre.bias_plan, r.g_lo, r.g_hi, h_sum, h_max);
    memcpy(sums, h_sum.data(), h_sum.size() * 8);
    memcpy(maxes, h_max.data(), h_max.size() * 8);
}
inline void prepare_normalization(PrepassSim &s, Uploader &up, const double *sums, const double *maxes, size_t n) {
    require_plan(s);
    if (n != (size_t)bias_chunks(s.pre.bias_plan)) throw Error("wrong number of partial sums");
    normalization_from_partials(s, up, s.pre.bias_plan, sums, maxes);
    s.pre.normalized = true;
}
// the chains over the rank's blocks, entered with its neighbours' states in_state[2] (forward chain from the left, reverse chain from the right); out_state[2]: what
// the neighbours' chains are entered with.  Called again for the same blocks, the run is kept and only what lies behind a replaced state runs again.
inline void prepare_sys_errors(PrepassSim &s, PrepassBackend &be, uint32_t block_lo, uint32_t block_hi, const uint32_t in_state[2], uint32_t out_state[2]) {
    require_plan(s);
    out_state[0] = in_state[0];                                     // a rank without blocks passes the states on
    out_state[1] = in_state[1];
    ChainRun &run = s.pre.run;
    if (!(run.valid && run.block_lo == block_lo && run.block_hi == block_hi)) {
        const ShardRange r = shard_range(s, block_lo, block_hi);
        s.passes = run_chains(s, be, kChainsSimulation, &r);
        run.block_lo = block_lo;
        run.block_hi = block_hi;
        run.pass_through = r.first_seq < 0;
        run.valid = true;
    }
    if (run.pass_through || !run.n_chunks) return;
    bool replaced = false;
    const int in_chain[2] = {run.edges.fwd_in_chain, run.edges.rev_in_chain};
    for (int k = 0; k < 2; ++k)
        if (in_chain[k] >= 0 && run.chains[(size_t)in_chain[k]].in_state != in_state[k]) {
            run.chains[(size_t)in_chain[k]].in_state = in_state[k];
            replaced = true;
        }
    if (replaced) {
        be.publish_chains(run);
        iterate_chains(run, be, run.passes);
        s.passes = run.passes;
    }
    const int64_t out_chunk[2] = {run.edges.fwd_out_chunk, run.edges.rev_out_chunk};
    for (int k = 0; k < 2; ++k) out_state[k] = out_chunk[k] >= 0 ? be.out_state(run, (int)((run.passes - 1) & 1), (size_t)out_chunk[k]) : 0u;
}
inline void prepare_finish(PrepassSim &s, PrepassBackend &be) {
    if (!(s.pre.planned && s.pre.run.valid)) throw Error("the sharded pre-pass has not run");
    if (!s.pre.normalized) throw Error("rsq_sim_prepare_normalization must run before rsq_sim_prepare_finish (the thresholds of the sieve come from it)");
    s.prepared_lo = s.pre.run.block_lo;                             // only these blocks' tracks are finished
    s.prepared_hi = s.pre.run.block_hi;
    if (s.has_variants) be.variant_sys_errors(s.pre.run);           // -V: the variants' bases inside the rank's strand windows, from the finished chains
    s.prepared = true;
    be.ready_to_simulate();
}

// Simulator::CreateSystematicErrorProfile (Simulator.cpp:2597-2653): both strands of every sequence, reverse first, as FASTQ.
// The reference reads sys_gc_range_ uninitialised in this mode (it is only set in Simulate, :2782); here it has that value.
inline void create_sys_error_profile(PrepassSim &s, Uploader &up, PrepassBackend &be, uint64_t seed, const char *path) {
    if (!s.has_ref) throw Error("a reference is needed to draw a systematic error profile");
    s.dev.seed = seed;
    set_sys_gc_range(s);
    run_chains(s, be, kChainsProfile);
    s.prepared = false;                                             // the simulation tracks were overwritten: prepare again before simulating
    std::string text;
    std::vector<uint8_t> dom, rate;
    for (uint32_t i = 0; i < s.dev.n_seqs; ++i)
        for (uint32_t strand = 2; strand--;) {
            const uint32_t L = s.seq_len[i];
            dom.resize(L);
            rate.resize(L);
            read_sys_track(up, (strand ? s.sys_rev : s.sys_fwd) + s.seq_base_off[i], L, dom.data(), rate.data());
            text += sys_error_fastq_record(s.ref_ids[i] + (strand ? " reverse" : " forward"), dom.data(), rate.data(), L);
        }
    write_text_file(path, text);
}

}  // namespace rsq
