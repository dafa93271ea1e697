// apt_front_end.cpp — see apt_front_end.hpp: the host-side design of a plan, the one reader of the plan's switches, the
// geometry of the TABLE / PHASE stage 1 with the PHASE table builder, and the choice of the front end.
#include "apt_front_end.hpp"

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

namespace apt {

// u32 overflow of rate * l (dsp.rs:86-93): the reference's message
static Error rate_overflow(Rate in, Rate out, LM lm)
{
    char buf[512];
    std::snprintf(buf, sizeof buf,
                  "Can't resample, looks like the sample rates do not have a big\n"
                  "                divisor in common. input_rate: %u, output_rate: %u, "
                  "l: %u, m: %u",
                  in.get_hz(), out.get_hz(), lm.l, lm.m);
    return Error{ErrorKind::RateOverflow, buf};
}

PlanDesign design_plan(const aptgpu_settings &settings, uint32_t input_rate, bool sync)
{
    PlanDesign d;
    // decode.rs:55 — u32 arithmetic; the reference would panic on overflow
    const uint64_t spr64 = static_cast<uint64_t>(PX_PER_ROW) * settings.work_rate;
    if (spr64 > 0xFFFFFFFFull) throw Error{ErrorKind::Invalid, "work_rate too large"};
    d.spr = static_cast<uint32_t>(spr64 / FINAL_RATE);
    // (the reference would divide by zero at decode.rs:142 / find nothing to sync on)
    if (d.spr == 0) throw Error{ErrorKind::Invalid, "work_rate too small"};

    const Rate in_rate = Rate::hz(input_rate);
    const Rate work_rate = Rate::hz(settings.work_rate);

    // ---- first resample: decode.rs:65-77 -> dsp.rs:62-126
    if (work_rate.get_hz() == 0) throw Error{ErrorKind::Internal, "Can't resample to 0Hz"};
    LowpassDcRemoval f1(Freq::hz(settings.resample_cutout, in_rate), settings.resample_atten,
                        Freq::hz(settings.resample_delta_freq, in_rate));
    const LM lm = interpolation_factors(in_rate, work_rate);
    d.l = lm.l;
    d.m = lm.m;
    if (lm.l > 1) {
        Rate interpolated{};
        if (!in_rate.checked_mul(lm.l, &interpolated)) throw rate_overflow(in_rate, work_rate, lm);
        f1.resample(in_rate, interpolated);
    }
    d.taps_resample = f1.design();

    // ---- demodulation constants: decode.rs:89, dsp.rs:360-363 (phi = 2*get_rad())
    const Freq carrier = Freq::hz(static_cast<float>(CARRIER_FREQ), work_rate);
    const float phi = 2.f * carrier.get_rad();
    d.cosphi2 = cosf(phi) * 2.f;
    d.sinphi = sinf(phi);

    // ---- low-pass: decode.rs:95-100
    const Freq cutout = Freq::pi_rad(static_cast<float>(FINAL_RATE) / static_cast<float>(work_rate.get_hz()));
    Lowpass f2(cutout, settings.demodulation_atten, cutout / 5.f);
    d.taps_lowpass = f2.design();

    // ---- sync geometry: decode.rs:204-216
    d.work_is_multiple = (work_rate.get_hz() % FINAL_RATE) == 0;
    d.pw = work_rate.get_hz() / FINAL_RATE;
    d.n_sync_taps = 38 * d.pw;
    d.md = static_cast<uint32_t>(static_cast<uint64_t>(d.spr) * 8 / 10);
    if (sync && d.work_is_multiple && static_cast<uint64_t>(d.md) * 8 > 160u * 1024u)
        throw Error{ErrorKind::Unsupported, "work_rate too large for the sync search (LDS)"};

    // ---- final resample to 4160 Hz: decode.rs:158-159
    const LM lm2 = interpolation_factors(work_rate, Rate::hz(FINAL_RATE));
    d.l2 = lm2.l;
    d.m2 = lm2.m;
    Rate tmp{};
    if (lm2.l > 1 && !work_rate.checked_mul(lm2.l, &tmp)) throw rate_overflow(work_rate, Rate::hz(FINAL_RATE), lm2);
    return d;
}

}  // namespace apt

namespace apt::gpu {

PlanSwitches read_plan_switches()
{
    auto flag = [](const char *name) {
        const char *e = std::getenv(name);
        return e ? static_cast<int>(static_cast<unsigned char>(e[0])) : -1;
    };
    PlanSwitches sw;
    sw.force_walk = flag("APTGPU_FORCE_WALK");
    if (const char *e = std::getenv("APTGPU_STREAMS")) sw.streams = std::max(1, std::min(std::atoi(e), 16));
    sw.fused_any = flag("APTGPU_FUSED_ANY");
    sw.phase_first = flag("APTGPU_PHASE_FIRST");
    sw.fast_mfma = flag("APTGPU_FAST_MFMA");
    sw.fused_pad = flag("APTGPU_FUSED_PAD");
    sw.quiet = flag("APTGPU_QUIET");
    sw.general_envelope = flag("APTGPU_GENERAL_ENVELOPE");
    sw.phase_balanced = flag("APTGPU_PHASE_BALANCED");
    sw.phase_tt = flag("APTGPU_PHASE_TT");
    sw.phase_wide = flag("APTGPU_PHASE_WIDE");
    if (const char *e = std::getenv("APTGPU_TABLE_LDS_KB")) sw.table_lds_kb = std::atol(e);
    sw.phase_identity = flag("APTGPU_PHASE_IDENTITY");
    return sw;
}

// ---- table-driven stage 1 (k_fused in TABLE mode)
bool fused_table_supported(uint32_t l, uint32_t m, uint32_t t1, uint32_t t2, uint32_t pw, long lds_kb, TableGeom *geom)
{
    constexpr uint32_t kThreads = 512, kPerThread = 13, kTile = kThreads * kPerThread;
    // 80 KB: two workgroups per CU.  APTGPU_TABLE_LDS_KB (A/B switch, <= 160) lets larger tables / tiles in at
    // one workgroup per CU.
    const uint32_t kLdsFloats = (lds_kb >= 16 && lds_kb <= 160) ? static_cast<uint32_t>(lds_kb) * 256u : 20480u;
    if (l < 2 || m == 0 || t1 == 0 || t2 != 37 || pw != 3) return false;  // (work-rate stages: standard profile)
    if (static_cast<uint64_t>(kTile + 4096) * m + l > 0x7fffffffull) return false;  // 32-bit in-tile index math
    TableGeom g{};
    g.l = l;
    g.m = m;
    g.jlim = 2 * ((t1 - 1) / 2) + 1;
    const uint32_t per_phase = (g.jlim + l - 1) / l;
    g.tpp = per_phase | 1u;  // odd stride: rows of consecutive phases start in different banks
    g.xt = (static_cast<uint32_t>((static_cast<uint64_t>(kTile) * m + l - 1) / l) + per_phase + 8 + 3) & ~3u;
    g.off_x = (l * g.tpp + 3u) & ~3u;
    g.step_q = static_cast<uint32_t>((static_cast<uint64_t>(kThreads) * m) / l);
    g.step_r = static_cast<uint32_t>((static_cast<uint64_t>(kThreads) * m) % l);
    g.jl_a = g.jlim / l;
    g.jl_b = g.jlim % l;
    if (static_cast<uint64_t>(g.off_x) + g.xt > kLdsFloats) return false;
    if (geom) *geom = g;
    return true;
}

// ---- phase-resident stage 1 (k_fused in PHASE mode)
namespace {
constexpr uint32_t kPhaseOutputs = 16;
constexpr uint32_t kPhaseMaxPerm = 8;
uint32_t phase_tpp(uint32_t l, uint32_t t1, bool stream = false)
{
    const uint32_t jlim = 2 * ((t1 - 1) / 2) + 1;
    return stream ? ((jlim + l - 1) / l + 15u) & ~15u : ((jlim + l - 1) / l + 3u) & ~3u;  // (streamed: whole chunks of 16)
}
// the tile of a PHASE workgroup (FusedGeom with TABLE geometry: whole groups of four halo threads either side)
struct PhaseTile {
    uint32_t pre_k, own_k;
};
constexpr PhaseTile phase_tile(uint32_t threads, uint32_t t2, uint32_t pw)
{
    const uint32_t pre = ((t2 + 1 + 12) / 13 + 3) / 4 * 4, post = ((38 * pw - 1 + 12) / 13 + 3) / 4 * 4;
    const uint32_t own = (threads - pre - post) / 4 * 4;
    return PhaseTile{pre * 13, own * 13};
}
uint32_t gcd_u32(uint32_t a, uint32_t b)
{
    while (b) {
        const uint32_t t = a % b;
        a = b;
        b = t;
    }
    return a;
}
// taps per branch a thread's registers hold (TPPM in k_fused)
uint32_t phase_tap_regs(uint32_t threads, uint32_t t2, uint32_t nq)
{
    if (threads == 1024) return 24;
    if (threads == 512) return 40;
    if (t2 == 43) return 28;
    return nq == 1 ? 76u : nq == 2 ? 36u : 20u;
}
// geometry for workgroups of `threads` (256: three per CU; 512: two; 1024: one) whose threads hold nq branches each
bool phase_geom(uint32_t threads, uint32_t nq, uint32_t l, uint32_t m, uint32_t t1, uint32_t t2, uint32_t pw, const PlanSwitches &sw,
                TableGeom *geom, bool stream = false)
{
    const uint32_t tile = threads * 13;
    if (nq == 1 ? l > threads : (l % nq != 0 || l / nq > threads || l <= threads)) return false;
    if (static_cast<uint64_t>(tile + 4096) * m + l > 0x7fffffffull) return false;  // 32-bit in-tile index math
    TableGeom g{};
    g.l = l;
    g.m = m;
    g.nq = nq;
    g.jlim = 2 * ((t1 - 1) / 2) + 1;
    const uint32_t per_phase = (g.jlim + l - 1) / l;
    if (!stream && per_phase > phase_tap_regs(threads, t2, nq)) return false;
    g.stream = stream ? 1u : 0u;
    g.tpp = phase_tpp(l, t1, stream);
    // outputs between a branch's consecutive outputs: as many whole periods of l as the threads hold (nq = 1), or l
    const uint32_t stride = nq == 1 ? l * (threads / l) : l;
    if ((tile + stride - 1) / stride > std::max(1u, kPhaseOutputs / nq)) return false;
    g.step_r = stride;
    g.step_q = static_cast<uint32_t>(static_cast<uint64_t>(stride) * m / l);  // exact: l divides stride
    // slot stride (TableGeom::sq): four / eight branches per thread — every thread takes slots, `threads` apart, and the
    // slots >= l do not exist; else l / nq slots of nq branches each (A/B switch, plan creation: APTGPU_PHASE_BALANCED=0 / 1)
    {
        // (default: where it measured faster — profiles/r06_phase_balanced_ab.txt: four branches at the standard and slow
        // profiles, eight at the fast one; not the fast profile's four (44 100 Hz) and sixteen, not two branches)
        const bool balanced = (sw.phase_balanced == '0' || sw.phase_balanced == '1') ? sw.phase_balanced == '1' : ((nq == 4 && t2 != 43) || nq == 8);
        g.sq = nq == 1 ? stride : (balanced ? threads : stride / nq);
    }
    // paired input tile: kPhaseOutputs / nq / 2 regions of off_x f2 entries — a branch's window starts at most
    // step_q + 4 entries into its region and is per_phase long
    g.off_x = g.step_q + per_phase + 8;
    // (the tile loader covers a region in 1024 / threads rounds; the fast profile's forms with four / eight branches per
    // thread — one or two regions only — in nine)
    if (g.off_x > ((t2 == 43 && nq > 2) ? 2304u : 1024u)) return false;
    g.xt = std::max(1u, kPhaseOutputs / nq / 2) * 2 * g.off_x;  // (sixteen branches: one region whose second half stays zero)
    // LDS: three 256-thread workgroups (53 KB each), two 512-thread ones (80 KB) or one of 1024 threads per CU
    if (g.xt > (threads == 256 ? 13600u : threads == 512 ? 20480u : 36000u)) return false;
    g.jl_a = g.jlim / l;
    g.jl_b = g.jlim % l;
    // the thread assignment lists: one per distinct tile phase rb = ((tile * own_k - pre_k) * m) mod l
    const PhaseTile pt = phase_tile(threads, t2, pw);
    const uint32_t step = static_cast<uint32_t>((static_cast<uint64_t>(pt.own_k) * m) % l);
    uint32_t nperm = step ? l / gcd_u32(l, step) : 1u;
    g.exact = (nperm <= kPhaseMaxPerm && (nperm & (nperm - 1)) == 0) ? 1u : 0u;
    if (!g.exact) nperm = 1;  // (then the list of tile 0 serves every tile: same results, more bank conflicts, divisions in the kernel)
    g.nthr = threads;
    g.nperm = nperm;
    g.perm_off = (l * g.tpp + 3u) & ~3u;
    g.cp_off = (g.perm_off + nperm * threads + 3u) & ~3u;
    g.tt_off = (g.cp_off + nperm * threads * nq + 3u) & ~3u;
    if (!g.exact || sw.phase_tt == '0') g.tt_off = 0;  // (A/B switch: 0 = phase-major rows only)
    for (g.perm_shift = 0; (1u << g.perm_shift) < nperm; ++g.perm_shift) {}
    if (g.exact) {
        g.xd = static_cast<uint32_t>(static_cast<uint64_t>(nperm) * pt.own_k * m / l);  // exact: the period's definition
        for (uint32_t r = 0; r < nperm; ++r) {
            const int64_t km = (static_cast<int64_t>(r) * pt.own_k - static_cast<int64_t>(pt.pre_k)) * static_cast<int64_t>(m);
            int64_t x0 = km / static_cast<int64_t>(l);
            if (x0 * static_cast<int64_t>(l) > km) --x0;  // floor
            g.x0r[r] = static_cast<int32_t>(x0);
            g.rbr[r] = static_cast<uint32_t>(km - x0 * static_cast<int64_t>(l));
        }
    }
    if (geom) *geom = g;
    return true;
}
// (kModeStrictPad2: whatever low-pass length its bound admits, the tile is the one the kernel is compiled for)
constexpr bool pad2_tile_is_fixed()
{
    for (uint32_t t2 = 1; t2 <= static_cast<uint32_t>(kPadT2Max); t2 += 2)
        if (phase_tile(256, t2, 3).pre_k != phase_tile(256, kPadT2Max, 3).pre_k || phase_tile(256, t2, 3).own_k != phase_tile(256, kPadT2Max, 3).own_k)
            return false;
    return true;
}
static_assert(pad2_tile_is_fixed(), "a PHASE tile that depends on the run-time low-pass length");
}  // namespace

uint32_t fused_phase_pad_t2(uint32_t t2, uint32_t pw, const PlanSwitches &sw)
{
    return sw.fused_pad == '0' ? 0u : fused_phase_pad_t2_bound(t2, pw);
}

bool fused_phase_supported(uint32_t l, uint32_t m, uint32_t t1, uint32_t t2, uint32_t pw, const PlanSwitches &sw, TableGeom *geom)
{
    if (l < 2 || m == 0 || t1 == 0) return false;
    // work-rate stages: the standard profile's (256 threads with one, two or four branches each; 512- and 1024-thread
    // workgroups), the fast profile's (256 threads, one branch)
    if (t2 == 43 && pw == 4)
        return phase_geom(256, 1, l, m, t1, t2, pw, sw, geom) || phase_geom(256, 4, l, m, t1, t2, pw, sw, geom) ||
               phase_geom(256, 8, l, m, t1, t2, pw, sw, geom) || phase_geom(256, 16, l, m, t1, t2, pw, sw, geom);
    // the slow profile's (61-tap low-pass, pixel width 5): its resampling filters (197 taps per branch at the sound-card
    // rates) do not fit the registers — the streamed form
    if (t2 == 61 && pw == 5)
        return phase_geom(256, 1, l, m, t1, t2, pw, sw, geom, true) || phase_geom(256, 2, l, m, t1, t2, pw, sw, geom, true) ||
               phase_geom(256, 4, l, m, t1, t2, pw, sw, geom, true);
    if (pw != 3) return false;
    if (t2 != 37) {
        // a tuned demodulation_atten: the instantiations compiled for a low-pass BOUND (kModeStrictPad2), 256 threads only
        // (geometry by the kernel's T2, the bound: phase_geom tells the profiles apart by their low-pass lengths)
        const uint32_t tb = fused_phase_pad_t2(t2, pw, sw);
        if (tb == 0) return false;
        return phase_geom(256, 1, l, m, t1, tb, pw, sw, geom) || phase_geom(256, 2, l, m, t1, tb, pw, sw, geom) ||
               phase_geom(256, 4, l, m, t1, tb, pw, sw, geom);
    }
    if (sw.phase_wide == '1' && (phase_geom(512, 1, l, m, t1, t2, pw, sw, geom) || phase_geom(1024, 1, l, m, t1, t2, pw, sw, geom)))
        return true;
    return phase_geom(256, 1, l, m, t1, t2, pw, sw, geom) || phase_geom(256, 2, l, m, t1, t2, pw, sw, geom) ||
           phase_geom(256, 4, l, m, t1, t2, pw, sw, geom) || phase_geom(512, 1, l, m, t1, t2, pw, sw, geom) ||
           phase_geom(1024, 1, l, m, t1, t2, pw, sw, geom);
}

uint32_t fused_phase_table_floats(const TableGeom &g)
{
    // (+ slack behind both tap tables: the streamed form prefetches one chunk past a row's end)
    const uint32_t base = g.tt_off ? g.tt_off : ((g.cp_off + g.nperm * g.nthr * (g.nq ? g.nq : 1u) + 3u) & ~3u);
    return base + (g.tt_off ? g.nperm * (g.nq ? g.nq : 1u) * g.tpp * g.nthr : 0u) + 64u * g.nthr / 4u + 80u;
}

// Thread -> branch-slot lists.  Thread t of a tile computes the outputs u, u + S, ... (S = step_r) for its slot u; the
// window of slot u starts c(u) = ceil((rb + u m) / l) entries into a region of the paired input tile, and every
// 8-byte LDS read of stage 1 is "entry c(u) + constant".  An 8-byte wave-read takes two cycles when the entries of each
// of its half-waves (lanes 0-31, 32-63) are distinct mod 32 — in any order, at any multiple of 32 — and half a cycle
// more per extra pass a half-wave needs (tools/ubench/lds_pat.hip, profiles/r05_ubench_lds_pat.txt: one pair 2.5, a pair
// in both halves 3.0); with slot = thread the starts advance m / l = 3.53 entries per lane at 44 100 Hz and up to
// four lanes of a half-wave share a residue (4.5 cycles measured).  The lists below deal the slots out over the
// half-waves so that as few of them as the residue class sizes allow need extra passes, for all of a thread's branches.  Which thread computes which slot changes
// nothing else: the tile loader indexes by thread, the results go to R in LDS by slot.
void fused_phase_table(const TableGeom &g, uint32_t t2, uint32_t pw, const float *coeff, float *table, const PlanSwitches &sw)
{
    const uint32_t l = g.l, tpp = g.tpp;
    for (uint32_t p = 0; p < l; ++p)
        for (uint32_t i = 0; i < tpp; ++i) {
            const uint64_t j = p + static_cast<uint64_t>(i) * l;
            table[static_cast<size_t>(p) * tpp + i] = j < g.jlim ? coeff[j] : 0.f;
        }
    const PhaseTile pt = phase_tile(g.nthr, t2, pw);
    const uint32_t nq = g.nq ? g.nq : 1u;
    const uint32_t S = g.sq;                           // slot stride = threads with work; thread slot u holds u + q S < step_r
    const uint32_t NH = 2 * ((S + 63) / 64);           // half-waves of the waves with work (the other waves skip stage 1's arithmetic)
    // does slot u's branch q exist?  (nq == 1: S = step_r, always; S = step_r / nq: always; S = threads: not the last ones)
    auto exists = [&](uint32_t u, uint32_t q) -> bool { return u + q * S < g.step_r; };
    auto branches_of = [&](uint32_t u) -> uint32_t {
        uint32_t n = 0;
        for (uint32_t q = 0; q < nq; ++q) n += exists(u, q) ? 1u : 0u;
        return n;
    };
    std::vector<uint32_t> list(g.nthr), ident_list(g.nthr);
    for (uint32_t t = 0; t < g.nthr; ++t) ident_list[t] = t < S ? t : 0xFFFFFFFFu;
    for (uint32_t r = 0; r < g.nperm; ++r) {
        const int64_t k0 = static_cast<int64_t>(r) * pt.own_k - static_cast<int64_t>(pt.pre_k);
        int64_t rb = (k0 * static_cast<int64_t>(g.m)) % static_cast<int64_t>(l);
        if (rb < 0) rb += l;
        // window start of slot u's branch q: its entry in a region, and that mod the 32 entry positions of the LDS banks
        auto ent = [&](uint32_t u, uint32_t q) -> uint32_t {  // (a slot that does not exist reads entry 0: every such lane the same one)
            if (!exists(u, q)) return 0u;
            return static_cast<uint32_t>((static_cast<uint64_t>(rb) + static_cast<uint64_t>(u + q * S) * g.m + l - 1) / l);
        };
        auto res = [&](uint32_t u, uint32_t q) -> uint32_t { return ent(u, q) & 31u; };
        // distinct entries among `have` (slots of one half-wave) that share the bank position of slot u's branch q and
        // differ from it (lanes that read the SAME entry are served together)
        auto rivals = [&](const std::vector<uint32_t> &have, uint32_t u, uint32_t q) -> uint32_t {
            const uint32_t e = ent(u, q);
            uint32_t n = 0;
            for (size_t i = 0; i < have.size(); ++i) {
                const uint32_t o = ent(have[i], q);
                if (o == e) return 0;  // u rides along with that lane
                if (((o ^ e) & 31u) != 0) continue;
                bool seen = false;
                for (size_t j = 0; j < i && !seen; ++j) seen = ent(have[j], q) == o;
                n += seen ? 0 : 1;
            }
            return n;
        };
        // passes a half-wave's read of branch q takes beyond the first: (most distinct entries on one bank position) - 1
        auto extra_of = [&](const std::vector<uint32_t> &have, uint32_t q) -> uint32_t {
            uint32_t mx = 0;
            for (uint32_t p = 0; p < 32; ++p) {
                std::vector<uint32_t> es;
                for (uint32_t u : have)
                    if (res(u, q) == p && std::find(es.begin(), es.end(), ent(u, q)) == es.end()) es.push_back(ent(u, q));
                mx = std::max<uint32_t>(mx, static_cast<uint32_t>(es.size()));
            }
            return mx ? mx - 1 : 0;
        };
        auto cost = [&](const std::vector<uint32_t> &ls) -> uint32_t {
            uint32_t total = 0;
            for (uint32_t h = 0; h < g.nthr / 32; ++h) {
                std::vector<uint32_t> have;
                for (uint32_t e = 0; e < 32; ++e)
                    if (ls[32 * h + e] < S) have.push_back(ls[32 * h + e]);
                for (uint32_t q = 0; q < nq; ++q) total += extra_of(have, q);
            }
            return total;
        };
        // greedy: slots of the largest residue classes (of branch 0) first, each to the half-wave where it adds the
        // fewest extra passes over all its branches; among equals, to the one where it meets the fewest rivals, then
        // to the emptiest
        // Slots with more branches first, into the first half-waves: a wave runs a branch when ANY of its lanes has it, so
        // the slots that have the last branch are kept together (l = 832: slots 0-63 in wave 0; a slot of another class
        // only lands in a class's half-waves when its own are full — results do not depend on the lists).
        std::vector<uint32_t> order(S);
        std::vector<uint32_t> csize(32, 0);
        for (uint32_t u = 0; u < S; ++u) ++csize[res(u, 0)];
        for (uint32_t u = 0; u < S; ++u) order[u] = u;
        std::stable_sort(order.begin(), order.end(), [&](uint32_t a, uint32_t b) {
            const uint32_t na = branches_of(a), nb = branches_of(b);
            return na != nb ? na > nb : csize[res(a, 0)] > csize[res(b, 0)];
        });
        std::vector<uint32_t> first_hw(nq + 1, 0);  // first half-wave of the slots with n branches
        {
            uint32_t before = 0;
            for (uint32_t nbr = nq; nbr >= 1; --nbr) {
                first_hw[nbr] = before / 32u;
                for (uint32_t u = 0; u < S; ++u) before += branches_of(u) == nbr ? 1u : 0u;
            }
        }
        std::vector<std::vector<uint32_t>> half(NH);
        std::vector<uint32_t> hextra(static_cast<size_t>(NH) * nq, 0);
        for (uint32_t u : order) {
            uint32_t best = 0;
            uint64_t best_key = ~0ull;
            const uint32_t h_lo = first_hw[branches_of(u)];
            bool room = false;
            for (uint32_t h = h_lo; h < NH; ++h) room = room || half[h].size() < 32;
            for (uint32_t h = room ? h_lo : 0u; h < NH; ++h) {
                if (half[h].size() >= 32) continue;
                uint32_t add = 0, mult = 0;
                for (uint32_t q = 0; q < nq; ++q) {
                    const uint32_t k = rivals(half[h], u, q);  // u would be entry number k + 1 on its bank position
                    if (k > hextra[static_cast<size_t>(h) * nq + q]) add += k - hextra[static_cast<size_t>(h) * nq + q];
                    mult += k;
                }
                const uint64_t key = (static_cast<uint64_t>(add) << 40) | (static_cast<uint64_t>(mult) << 20) | half[h].size();
                if (key < best_key) {
                    best_key = key;
                    best = h;
                }
            }
            for (uint32_t q = 0; q < nq; ++q) {
                uint32_t &hx = hextra[static_cast<size_t>(best) * nq + q];
                hx = std::max(hx, rivals(half[best], u, q));
            }
            half[best].push_back(u);
        }
        for (uint32_t t = 0; t < g.nthr; ++t) list[t] = 0xFFFFFFFFu;
        for (uint32_t h = 0; h < NH; ++h)
            for (uint32_t e = 0; e < half[h].size(); ++e) list[32 * h + e] = half[h][e];
        const bool use_ident = sw.phase_identity == '1' || cost(ident_list) <= cost(list);
        const std::vector<uint32_t> &chosen = use_ident ? ident_list : list;
        std::memcpy(table + g.perm_off + static_cast<size_t>(r) * g.nthr, chosen.data(), g.nthr * sizeof(uint32_t));
        // window start and branch of every slot of every thread (the kernel reads them when g.exact)
        std::vector<uint32_t> cp(static_cast<size_t>(g.nthr) * nq, 0u);
        for (uint32_t t = 0; t < g.nthr; ++t)
            for (uint32_t q = 0; q < nq; ++q) {
                const bool have = chosen[t] < S && exists(chosen[t], q);  // (else: window start 0, branch 0 — read, never stored)
                const uint64_t v = static_cast<uint64_t>(rb) + static_cast<uint64_t>(have ? chosen[t] + q * S : 0u) * g.m;
                const uint64_t c = have ? (v + l - 1) / l : 0u, ph = have ? c * l - v : 0u;
                cp[static_cast<size_t>(t) * nq + q] = static_cast<uint32_t>(c) | (static_cast<uint32_t>(ph) << 16);
            }
        std::memcpy(table + g.cp_off + static_cast<size_t>(r) * g.nthr * nq, cp.data(), cp.size() * sizeof(uint32_t));
        if (g.tt_off) {
            // the taps in thread order: [r][q][e][t][4]
            for (uint32_t q = 0; q < nq; ++q)
                for (uint32_t e = 0; e < tpp / 4; ++e)
                    for (uint32_t t = 0; t < g.nthr; ++t) {
                        const uint32_t ph = cp[static_cast<size_t>(t) * nq + q] >> 16;
                        float *dst = table + g.tt_off + (((static_cast<size_t>(r) * nq + q) * (tpp / 4) + e) * g.nthr + t) * 4;
                        const bool have = chosen[t] < S && exists(chosen[t], q);
                        for (uint32_t k = 0; k < 4; ++k) dst[k] = have ? table[static_cast<size_t>(ph) * tpp + 4 * e + k] : 0.f;
                    }
        }
    }
}

// ---- which front end serves a plan
FrontEnd select_front_end(uint32_t l, uint32_t m, uint32_t t1, uint32_t t2, uint32_t pw, int mode, bool work_is_multiple,
                          bool export_filtered, const PlanSwitches &sw)
{
    FrontEnd fe;
    // (not with export_resample_filtered: the fused kernels decimate at t = off + k m, the flag moves the phase —
    // dsp.rs:265-273 — and work_len_for() follows the flag; the unfused k_resample_at path serves such a plan)
    const bool fusable = l > 1 && work_is_multiple && !export_filtered;
    // APTGPU_MODE_FAST permits deviations within the stated tolerance; where no fast kernel exists
    // (other rates / profiles) the strict kernels serve it
    const bool eligible = (mode == APTGPU_MODE_STRICT || mode == APTGPU_MODE_FAST) && fusable;
    const bool spec = eligible && sw.fused_any != '1';  // a specialised kernel may serve it
    const bool exact = fused_exact_variant(l, m, t1, t2, pw, kModeStrict) != kFusedNone;  // a stock geometry
    // APTGPU_MODE_FAST on the matrix cores (kModeMfma: 48 / 96 kHz at the standard profile, ANY tap count its K holds).
    // Measured at parity with / a few percent behind the VALU fast kernels at the stock tap counts (fast
    // mode is bound by the tile's HBM round trip, not by the FIRs), so it serves the plans those kernels cannot — a tuned
    // resample_atten / resample_delta_freq, which changes the tap count — and, APTGPU_FAST_MFMA=1 (A/B switch, tests), all
    // it has an instantiation for; APTGPU_FAST_MFMA=0 switches it off.
    const bool mfma_want = sw.fast_mfma >= 0 ? sw.fast_mfma == '1' : !exact;
    const bool mfma = spec && mode == APTGPU_MODE_FAST && mfma_want && fused_mfma_fits(l, m, t1, t2, pw);
    // a tap count no specialised kernel is compiled for (a tuned resample_atten / resample_delta_freq): the strict kernel
    // compiled for a tap-count BOUND, its table zero-padded (kModeStrictPad; APTGPU_FUSED_PAD=1 forces it for the stock
    // counts too, =0 switches it off: A/B, tests)
    const bool pad_want = sw.fused_pad >= 0 ? sw.fused_pad == '1' : !exact;
    const uint32_t pad_t1 = (spec && !mfma && pad_want) ? fused_pad_t1_bound(l, m, t1, t2, pw) : 0u;
    if (spec && (exact || mfma || pad_t1 != 0)) {
        fe.kind = FrontEndKind::Split;
        fe.mfma = mfma;
        fe.pad_t1 = pad_t1;
        fe.pad_t2 = pad_t1 ? fused_pad_t2_bound(l, m, t2, pw) : 0u;  // (a tuned demodulation_atten)
    }
    // (where both the table-driven and the phase-resident stage 1 exist, the latter: since round 5 — thread assignment
    // lists, interior tile loads, pipelined taps, two / four branches per thread — it is the faster one at every rate
    // measured (8 / 11.025 / 16 / 32 kHz: 0.60 / 0.64 / 0.71 / 0.95 against 0.70 / 0.68 / 0.94 / 1.56 ms per 16 recordings,
    // profiles/r05_sweeps.txt); APTGPU_PHASE_FIRST=0 (tests) puts the table-driven form first again)
    else if (spec && sw.phase_first != '0' && fused_phase_supported(l, m, t1, t2, pw, sw, &fe.geom))
        fe.kind = FrontEndKind::Phase;
    else if (spec && fused_table_supported(l, m, t1, t2, pw, sw.table_lds_kb, &fe.geom))
        fe.kind = FrontEndKind::Table;  // (11 025 Hz)
    else if (spec && fused_phase_supported(l, m, t1, t2, pw, sw, &fe.geom))
        fe.kind = FrontEndKind::Phase;  // (44 100 Hz)
    else if (eligible && fused_any_supported(l, m, t1, t2, pw))
        fe.kind = FrontEndKind::Any;
    // (a tuned low-pass on the PHASE kernels: strict kModeStrictPad2 instantiations only)
    if (fe.kind == FrontEndKind::Phase) fe.pad_t2 = fused_phase_pad_t2(t2, pw, sw);
    fe.fast = mode == APTGPU_MODE_FAST &&
              ((fe.kind == FrontEndKind::Split && pad_t1 == 0 && (mfma || fused_exact_variant(l, m, t1, t2, pw, kModeFast) != kFusedNone)) ||
               fe.kind == FrontEndKind::Table || (fe.kind == FrontEndKind::Phase && fe.pad_t2 == 0));
    // fp16-tap mode inside the specialised fused kernel where one exists (else the generic kernel)
    if (mode == APTGPU_MODE_FP16_TAPS && fusable && fused_exact_variant(l, m, t1, t2, pw, kModeF16Taps) != kFusedNone) {
        fe.kind = FrontEndKind::Split;
        fe.f16 = true;
    }
    fe.kmode = fe.f16 ? kModeF16Taps : fe.mfma ? kModeMfma : fe.pad_t1 ? kModeStrictPad : fe.fast ? kModeFast : kModeStrict;
    if (!fe.writes_planes()) return fe;

    const TableGeom &g = fe.geom;
    for (int i16 = 0; i16 < 2; ++i16) {
        FusedVariant v = fe.kind == FrontEndKind::Split ? fused_split_variant(l, m, t1, t2, pw, fe.kmode, i16 != 0)
                         : fe.kind == FrontEndKind::Table ? fused_table_variant(fe.kmode)
                                                          : fused_phase_variant(g.nq, g.nthr, g.stream != 0, t2, pw, fe.kmode);
        if (v != kFusedNone && i16 && !kFusedVariants[v].i16) v = kFusedNone;
        fe.variant[i16] = v;
    }
    if (fe.variant[0] == kFusedNone) throw Error{ErrorKind::Internal, "fused front end: no kernel for this geometry"};
    if (fe.kind == FrontEndKind::Table) fe.lds_floats = static_cast<size_t>(g.off_x) + g.xt;
    if (fe.kind == FrontEndKind::Phase) {
        // the tile and its LDS by the instantiation's own T2 and mode, as the kernel computes them — which must be what
        // the plan's low-pass length gives (one branch per thread: the paired tile goes through LDS in two halves)
        const FusedVariantRow &row = kFusedVariants[fe.variant[0]];
        const int nq = static_cast<int>(g.nq ? g.nq : 1u);
        const bool halves = phase_halves(nq, g.stream != 0, static_cast<int>(g.nthr), row.t2, row.mode == kModeFast);
        const bool fast_asked = fe.kmode == kModeFast && !(pw == 3 && t2 != 37);  // (a tuned low-pass: strict whatever the mode)
        const PhaseTile a = phase_tile(g.nthr, t2, pw), b = phase_tile(g.nthr, static_cast<uint32_t>(row.t2), static_cast<uint32_t>(row.pw));
        if (halves != phase_halves(nq, g.stream != 0, static_cast<int>(g.nthr), static_cast<int>(t2), fast_asked) || a.pre_k != b.pre_k ||
            a.own_k != b.own_k)
            throw Error{ErrorKind::Internal, "fused front end: the tile of the low-pass length differs from the kernel's"};
        fe.lds_floats = halves ? g.xt / 2 : g.xt;
    }
    return fe;
}

}  // namespace apt::gpu
