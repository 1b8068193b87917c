// rng_probe.hpp — TESTS ONLY.  A small script interpreter over the project's own random generators (rng.hpp: Mt19937, Philox;
// kuka_group.hpp: GroupMt, Lane0Rng, GroupPhilox, GroupActions): every value a script draws is written out as raw bits, so a test
// can hold the streams to numpy's RandomState / the Philox4x32-10 definition word for word.  One text, two builds: the device
// kernels of rng_probe.hip (srlhip_selftest_rng) and the host harness of kuka_hostcheck.cpp (hostcheck_rng_probe, the 16 lanes
// of a group as lockstep fibers).  No generator arithmetic is restated here: the adaptors below only route the script's ops to
// the generators' own members and move their persistent state through memory the way a kernel boundary does.
#pragma once
#include "kuka_group.hpp"

namespace srl {
namespace rngprobe {
namespace grp = kuka::grp;

enum Gen { GEN_MT = 0, GEN_GROUP_MT = 1, GEN_LANE0_MT = 2, GEN_PHILOX = 3, GEN_GROUP_PHILOX = 4, GEN_GROUP_ACTIONS = 5, GEN_COUNT = 6 };
// script rows are (op, index of the op's first argument in args[], repeat count)
enum Op {
    OP_U32 = 0,         // one tempered MT word; Philox: the four words of one block (four values)
    OP_DOUBLE01 = 1,
    OP_UNIFORM = 2,     // args: lo, hi
    OP_NORMAL = 3,      // args: loc, scale
    OP_BOUNDED = 4,     // args: r (a whole number below 2^32) -> a draw from [0, r]
    OP_STORE_LOAD = 5,  // the generator goes back to its state in memory and is loaded again, as at a kernel boundary
    OP_SET_CTR = 6,     // Philox family; args: offset (whole number) -> counter = the env's start counter + offset, generator re-initialised
    OP_COUNT = 7
};
constexpr int kMtStateWords = MT_N + 3;      // state_in / state_out of the MT forms, uint64 per env: 624 words, mti, has_gauss, gauss bits
constexpr int64_t kMaxValues = 1 << 20, kMaxSkip = 1 << 20;

SRL_HD constexpr bool is_group(int gen) { return gen == GEN_GROUP_MT || gen == GEN_LANE0_MT || gen == GEN_GROUP_PHILOX || gen == GEN_GROUP_ACTIONS; }
SRL_HD constexpr bool is_mt(int gen) { return gen == GEN_MT || gen == GEN_GROUP_MT || gen == GEN_LANE0_MT; }
SRL_HD bool op_allowed(int gen, int op) {
    if (op < 0 || op >= OP_COUNT) return false;
    if (op == OP_STORE_LOAD) return true;
    if (op == OP_SET_CTR) return !is_mt(gen);
    if (gen == GEN_GROUP_ACTIONS) return op == OP_BOUNDED;                   // GroupActions has one draw: next(m)
    if (op == OP_U32) return gen == GEN_MT || gen == GEN_GROUP_MT || gen == GEN_PHILOX;      // (Lane0Rng / GroupPhilox hand out no raw words)
    return true;
}
SRL_HD int values_of(int gen, int op) { return op >= OP_STORE_LOAD ? 0 : (op == OP_U32 && gen == GEN_PHILOX ? 4 : 1); }

// what a probe launch works on (device pointers in the kernels, host pointers in the harness)
struct Args {
    Mt19937View mt;              // MT forms: the envs' state, seeded or installed beforehand
    const uint32_t *keys;        // Philox forms: [2][n] key words
    uint64_t *ctr;               // Philox forms: [n] counters, in and out
    int32_t stream;              // per-lane Philox: 0 / 1
    int32_t n, n_ops;
    const uint8_t *mask;         // [n] or null: envs with mask 0 never draw
    const int32_t *script;       // [n_ops][3]
    const double *args;
    const int32_t *skip;         // [n]: raw words (MT) / blocks (Philox) / normal(0, 1) (GroupPhilox) / next(5) (GroupActions) draws env e throws away first
    uint64_t *out;               // [n][lanes][values]
    int64_t values;              // per lane
};

SRL_HD uint64_t bits_of(double x) { union { double d; uint64_t u; } c; c.d = x; return c.u; }

// ---- adaptors: one per generator form --------------------------------------------------------------------------------
struct MtAd {
    Mt19937 m; const Args *a; int64_t e;
    SRL_G void begin(const Args &aa, int64_t ee) { a = &aa; e = ee; m.load(aa.mt, ee); }
    SRL_G void skip(int k) { for (int i = 0; i < k; i++) (void)m.u32(); }
    SRL_G void u32(uint64_t *o) { o[0] = m.u32(); }
    SRL_G double double01() { return m.double01(); }
    SRL_G double uniform(double lo, double hi) { return m.uniform(lo, hi); }
    SRL_G double normal(double loc, double scale) { return m.normal(loc, scale); }
    SRL_G uint32_t bounded(uint32_t r) { return m.bounded(r); }
    SRL_G void store_load() { m.store(a->mt, e); m.load(a->mt, e); }
    SRL_G void set_ctr(uint64_t) {}
    SRL_G void end() { m.store(a->mt, e); }
};
struct GroupMtAd {
    grp::GroupMt r; const Args *a; int64_t e;
    SRL_G void begin(const Args &aa, int64_t ee) { a = &aa; e = ee; r.load(aa.mt, ee); }
    SRL_G void skip(int k) { for (int i = 0; i < k; i++) (void)r.u32(); }
    SRL_G void u32(uint64_t *o) { o[0] = r.u32(); }
    SRL_G double double01() { return r.double01(); }
    SRL_G double uniform(double lo, double hi) { return r.uniform(lo, hi); }
    SRL_G double normal(double loc, double scale) { return r.normal(loc, scale); }
    SRL_G uint32_t bounded(uint32_t m) { return r.bounded(m); }
    // the lead lane stores (kuka_tree_kernels.hpp: `if (lead) rng0.store(rs.mt, e)`), every lane loads: a partly consumed window is dropped
    SRL_G void store_load() { if (grp::lane_id() == 0) r.store(a->mt, e); grp::sync_scratch(); r.load(a->mt, e); grp::sync_scratch(); }
    SRL_G void set_ctr(uint64_t) {}
    SRL_G void end() { if (grp::lane_id() == 0) r.store(a->mt, e); }
};
struct Lane0MtAd {        // the lumped lane-group kernels: every lane loads the env's generator, lane 0 draws, the row receives the value
    Mt19937 m; grp::Lane0Rng<Mt19937> r; const Args *a; int64_t e;
    SRL_G void begin(const Args &aa, int64_t ee) { a = &aa; e = ee; m.load(aa.mt, ee); r.r = &m; r.own = grp::lane_id() == 0; }
    SRL_G void skip(int k) { if (r.own) for (int i = 0; i < k; i++) (void)m.u32(); }
    SRL_G void u32(uint64_t *o) { o[0] = 0; }
    SRL_G double double01() { return r.double01(); }
    SRL_G double uniform(double lo, double hi) { return r.uniform(lo, hi); }
    SRL_G double normal(double loc, double scale) { return r.normal(loc, scale); }
    SRL_G uint32_t bounded(uint32_t mm) { return r.bounded(mm); }
    SRL_G void store_load() { if (r.own) m.store(a->mt, e); grp::sync_scratch(); m.load(a->mt, e); grp::sync_scratch(); }
    SRL_G void set_ctr(uint64_t) {}
    SRL_G void end() { if (r.own) m.store(a->mt, e); }
};
struct PhiloxAd {
    Philox p; const Args *a; int64_t e; uint64_t ctr0;
    SRL_G void begin(const Args &aa, int64_t ee) {
        a = &aa; e = ee; ctr0 = aa.ctr[ee];
        p.k0 = aa.keys[ee]; p.k1 = aa.keys[aa.n + ee]; p.ctr = ctr0; p.stream = (uint32_t)aa.stream;
    }
    SRL_G void skip(int k) { for (int i = 0; i < k; i++) { uint32_t o[4]; p.block(o); } }
    SRL_G void u32(uint64_t *o) { uint32_t w[4]; p.block(w); for (int i = 0; i < 4; i++) o[i] = w[i]; }
    SRL_G double double01() { return p.double01(); }
    SRL_G double uniform(double lo, double hi) { return p.uniform(lo, hi); }
    SRL_G double normal(double loc, double scale) { return p.normal(loc, scale); }
    SRL_G uint32_t bounded(uint32_t r) { return p.bounded(r); }
    SRL_G void store_load() { a->ctr[e] = p.ctr; p.ctr = a->ctr[e]; }
    SRL_G void set_ctr(uint64_t off) { p.ctr = ctr0 + off; }
    SRL_G void end() { a->ctr[e] = p.ctr; }
};
// the group forms start from init(key, counter) as the kernels do at their top, and persist the counter through the lead lane
template <class R> struct GroupCtrAd {
    R r; const Args *a; int64_t e; uint64_t ctr0;
    SRL_G void begin(const Args &aa, int64_t ee) { a = &aa; e = ee; ctr0 = aa.ctr[ee]; r.init(aa.keys[ee], aa.keys[aa.n + ee], ctr0); }
    SRL_G void u32(uint64_t *o) { o[0] = 0; }
    SRL_G void store_load() {
        if (grp::lane_id() == 0) a->ctr[e] = r.p.ctr;
        grp::sync_scratch();
        r.init(a->keys[e], a->keys[a->n + e], a->ctr[e]);
        grp::sync_scratch();
    }
    SRL_G void set_ctr(uint64_t off) { r.init(a->keys[e], a->keys[a->n + e], ctr0 + off); }
    SRL_G void end() { if (grp::lane_id() == 0) a->ctr[e] = r.p.ctr; }
};
// skip: draws thrown away before the script, so that the rows of one wavefront stand at different offsets of their 16-counter batches
struct GroupPhiloxAd : GroupCtrAd<grp::GroupPhilox> {
    SRL_G void skip(int k) { for (int i = 0; i < k; i++) (void)r.normal(0.0, 1.0); }
    SRL_G double double01() { return r.double01(); }
    SRL_G double uniform(double lo, double hi) { return r.uniform(lo, hi); }
    SRL_G double normal(double loc, double scale) { return r.normal(loc, scale); }
    SRL_G uint32_t bounded(uint32_t m) { return r.bounded(m); }
};
struct GroupActionsAd : GroupCtrAd<grp::GroupActions> {
    SRL_G void skip(int k) { for (int i = 0; i < k; i++) (void)r.next(5u); }
    SRL_G double double01() { return 0.0; }
    SRL_G double uniform(double, double) { return 0.0; }
    SRL_G double normal(double, double) { return 0.0; }
    SRL_G uint32_t bounded(uint32_t m) { return (uint32_t)r.next(m); }
};
template <int GEN> struct AdaptorOf;
template <> struct AdaptorOf<GEN_MT> { using type = MtAd; };
template <> struct AdaptorOf<GEN_GROUP_MT> { using type = GroupMtAd; };
template <> struct AdaptorOf<GEN_LANE0_MT> { using type = Lane0MtAd; };
template <> struct AdaptorOf<GEN_PHILOX> { using type = PhiloxAd; };
template <> struct AdaptorOf<GEN_GROUP_PHILOX> { using type = GroupPhiloxAd; };
template <> struct AdaptorOf<GEN_GROUP_ACTIONS> { using type = GroupActionsAd; };

// The interpreter: env e's script on the calling lane (`lane` of `lanes`: 0 of 1 for the per-env forms).  The caller has already
// applied the kernels' guard (no call for a masked-out env or a shadow row) and checked the script against op_allowed / a.values.
template <int GEN> SRL_G void run_script(const Args &a, int64_t e, int lane, int lanes) {
    typename AdaptorOf<GEN>::type g;
    g.begin(a, e);
    g.skip(a.skip[e]);
    uint64_t *out = a.out + (e * lanes + lane) * a.values;
    int64_t k = 0;
    for (int o = 0; o < a.n_ops; o++) {
        const int op = a.script[3 * o], rep = a.script[3 * o + 2];
        const double *arg = a.args + a.script[3 * o + 1];
        for (int i = 0; i < rep; i++) {
            switch (op) {
                case OP_U32: g.u32(out + k); k += values_of(GEN, OP_U32); break;
                case OP_DOUBLE01: out[k++] = bits_of(g.double01()); break;
                case OP_UNIFORM: out[k++] = bits_of(g.uniform(arg[0], arg[1])); break;
                case OP_NORMAL: out[k++] = bits_of(g.normal(arg[0], arg[1])); break;
                case OP_BOUNDED: out[k++] = g.bounded((uint32_t)arg[0]); break;
                case OP_STORE_LOAD: g.store_load(); break;
                default: g.set_ctr((uint64_t)arg[0]); break;
            }
        }
    }
    g.end();
}

// Host-side check of a script (both builds): < 0 = refused, else the values one lane writes.
inline int64_t script_values(int gen, const int32_t *script, int n_ops, const double *args, int n_args) {
    if (gen < 0 || gen >= GEN_COUNT || n_ops < 0 || n_args < 0 || (n_ops && !script) || (n_args && !args)) return -1;
    int64_t v = 0;
    for (int o = 0; o < n_ops; o++) {
        const int op = script[3 * o], ai = script[3 * o + 1], rep = script[3 * o + 2];
        if (!op_allowed(gen, op) || rep < 0) return -1;
        const bool whole = op == OP_BOUNDED || op == OP_SET_CTR;
        const int need = op == OP_UNIFORM || op == OP_NORMAL ? 2 : (whole ? 1 : 0);
        if (ai < 0 || ai + need > n_args) return -1;
        if (whole) {        // whole numbers that the casts of run_script hold exactly
            const double x = args[ai], lim = op == OP_BOUNDED ? 4294967296.0 : 9007199254740992.0;
            if (!(x >= 0.0 && x < lim) || x != (double)(uint64_t)x) return -1;
        }
        v += (int64_t)rep * values_of(gen, op);
        if (v > kMaxValues) return -1;
    }
    return v;
}

}  // namespace rngprobe
}  // namespace srl
