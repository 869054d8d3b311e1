// The dispatch policy of memhip_attn_fwd / memhip_attn_bwd (DESIGN.md section 4 summarises it; these functions are the truth).
// Every shape test, option test and LDS-budget comparison of the attention entry points is here, once; the launchers obey.
#include "attn_plan.hpp"

namespace memhip {
namespace {

constexpr int HD = 64;

int cdiv(int a, int b) { return (a + b - 1) / b; }

bool attn16_fits(const AttnShape& p) { return p.window_h == 14 && p.window_w == 14 && p.T == 197; }
// windows 40 / 20 wide and longer than 256 tokens: the widths attn_win.hip instantiates
bool attn_win_fits(const AttnShape& p) {
  return p.T > 256 && (p.window_w == 40 || p.window_w == 20) && p.T == p.window_h * p.window_w + 1;
}

void push(AttnPlan& a, int kernel, int gx, int gy, int gz, int block, int64_t lds) {
  a.l[a.count++] = AttnLaunch{kernel, gx, gy, gz, block, (int32_t)lds};
}
// no family takes the shape: `family` stays the last one tried
AttnPlan over_budget(AttnPlan a, int family, int64_t lds) {
  a.family = family;
  a.count = 0;
  a.lds_over = (int32_t)(lds < INT32_MAX ? lds : INT32_MAX);
  return a;
}
bool fits(int64_t lds) { return lds <= kMaxLds; }

// ---- attn16.hip.  Workgroups per head: one workgroup per CU (LDS), as many as fit in one round.
// Quirk kept: a stream that reports no CUs is planned as 256 (pick_spb and nwg16 only; the win grids take the count as it is).
int cus_or_256(int stream_cus) { return stream_cus > 0 ? stream_cus : 256; }
int nwg16(const AttnShape& p, int stream_cus) {
  const int n = cus_or_256(stream_cus) / p.heads;
  return n < 1 ? 1 : (n > p.B ? p.B : n);
}

// ---- attn.hip.  Samples per workgroup.  One workgroup is resident per CU (LDS), so a grid of more than #CUs
// workgroups runs a second, nearly empty round: ceil(256*12/256) = 12 samples per workgroup gives
// 22 * 12 = 264 workgroups on 256 CUs, i.e. T(12) + T(4) -- 13 gives 240 workgroups and T(13)
// (measured: forward 156 -> 130 us, backward 603 -> 503 us per layer).  Dealing (head, sample) pairs
// perfectly evenly (12 per workgroup, runs crossing into the next head) was tried and is no faster:
// the crossing workgroups pay the per-head setup twice.  Smallest count for which the grid fits one
// round.  Quirk kept: capped at 16 samples (the table-gradient buckets are sized for that).
int pick_spb(const AttnShape& p, int stream_cus) {
  const int num_cu = cus_or_256(stream_cus);
  for (int spb = 1; spb <= 16; ++spb)
    if ((long long)cdiv(p.B, spb) * p.heads <= num_cu) return spb;
  return 16;
}

// ---- attn_win.hip.  Samples per workgroup: the table set-up is paid once per workgroup; keep the grid a few rounds of the
// chip deep.  Quirk kept: 6 * cus workgroups, the sample slots halved until the grid is below that.
int win_slots(int B, long long per_slot, int stream_cus) {
  int nb = B;
  while (nb > 1 && per_slot * nb > 6LL * stream_cus) nb = (nb + 1) / 2;
  return nb;
}
// Quirk kept: grids are rounded up to 8 workgroups per XCD map (win_wg, attn_win_common.hpp): 8 * ceil(pairs / 8) * groups
int win_grid(int heads, int slots, int groups) { return 8 * ((heads * slots + 7) / 8) * groups; }

// slots per row of the stored dS (whole chunks) -- the one expression behind the workspace size and the workspace condition
template <int WW> int win_qs(int Wh) { return WinGeo<WW>::CT * cdiv(Wh, WinGeo<WW>::RPC); }
int win_qs(const AttnShape& p) { return p.window_w == 40 ? win_qs<40>(p.window_h) : win_qs<20>(p.window_h); }
int64_t win_ws_need(const AttnShape& p, int TP) { return (int64_t)p.B * p.heads * TP * win_qs(p) * 2; }

struct WinLds { int64_t fwd, kv, q, kvs, kvs0, qs; };
template <int WW> WinLds win_lds(int Wh) {
  using G = WinGeo<WW>;
  const int64_t NBP = ((2 * Wh - 1) * G::P + 3) & ~3, imgs = (int64_t)4 * G::CT * 128;
  WinLds w;
  w.fwd = (NBP + G::CQ) * 4 + imgs;
  w.kv = (NBP + G::CQ + 4 * G::CT + 8 * HD) * 4 + imgs;
  w.q = (2 * (NBP + G::CQ) + 8 * HD) * 4 + imgs;
  w.kvs = (2 * (NBP + 2 * G::CQ) + 16 + 4 * G::CT + 8 * HD) * 4 + imgs;     // with the table gradient
  w.kvs0 = ((NBP + 2 * G::CQ) + 16 + 4 * G::CT + 8 * HD) * 4 + imgs;        // without
  w.qs = (int64_t)8 * HD * 4 + (int64_t)3 * 5 * 64 * 128;
  return w;
}
WinLds win_lds(const AttnShape& p) { return p.window_w == 40 ? win_lds<40>(p.window_h) : win_lds<20>(p.window_h); }

// ---- attn_stream.hip: key / query chunks of 32-token blocks per kernel
constexpr int kFwdCKB = 4, kKvCKB = 4, kQCKB = 2;
int64_t stream_lds_fwd(const AttnShape& p) {
  constexpr int CT = kFwdCKB * 32;
  return (int64_t)4 * CT * 128 + (int64_t)(rel_geom(p.window_h, p.window_w).len + 2 * (cdiv(p.T, CT) * CT)) * 4 + 32;
}

AttnPlan start(const AttnShape& p) {
  AttnPlan a = {};
  a.groups = (cdiv(p.T, 32) + 7) / 8;
  return a;
}

}  // namespace

int64_t attn_bwd_win_workspace(int B, int T, int heads, int window_h, int window_w) {
  const AttnShape p = {B, T, heads, window_h, window_w};
  return attn_win_fits(p) ? win_ws_need(p, cdiv(T, 32) * 32) : 0;
}

AttnPlan attn_plan_fwd(const AttnShape& p, int stream_cus, const AttnOptions& o) {
  AttnPlan a = start(p);
  const int nkb = cdiv(p.T, 32), glen = rel_geom(p.window_h, p.window_w).len;
  if (o.attn16 && attn16_fits(p)) {
    a.family = MEMHIP_ATTN_16;
    a.nwg = nwg16(p, stream_cus);
    push(a, MEMHIP_ATTN_K_FWD16, a.nwg * p.heads, 1, 1, kAttn16ThreadsFwd, kAttn16LdsFwd);
    return a;
  }
  if (nkb <= 8) {
    const int64_t sm = (int64_t)4 * nkb * 32 * 128 + (int64_t)(glen + 2 * nkb * 32) * 4 + 32;
    if (!fits(sm)) return over_budget(a, MEMHIP_ATTN_SMALL, sm);
    a.family = MEMHIP_ATTN_SMALL;
    a.n = nkb;
    a.spb = pick_spb(p, stream_cus);
    push(a, MEMHIP_ATTN_K_FWD, cdiv(p.B, a.spb) * p.heads, 1, 1, 512, sm);
    return a;
  }
  // any non-zero attn_win selects the slot-layout family
  if (o.attn_win && attn_win_fits(p) && fits(win_lds(p).fwd)) {
    a.family = MEMHIP_ATTN_WIN;
    a.ww = p.window_w;
    a.nbz = win_slots(p.B, (long long)a.groups * p.heads, stream_cus);
    push(a, MEMHIP_ATTN_K_FWD_WIN, win_grid(p.heads, a.nbz, a.groups), 1, 1, 512, win_lds(p).fwd);
    return a;
  }
  const int64_t sm = stream_lds_fwd(p);
  if (!fits(sm)) return over_budget(a, MEMHIP_ATTN_STREAM, sm);
  a.family = MEMHIP_ATTN_STREAM;
  push(a, MEMHIP_ATTN_K_FWD_STREAM, a.groups, p.heads, p.B, 512, sm);
  return a;
}

AttnPlan attn_plan_bwd(const AttnShape& p, const AttnBwdFlags& f, int stream_cus, const AttnOptions& o) {
  AttnPlan a = start(p);
  const int nkb = cdiv(p.T, 32), TP = nkb * 32, glen = rel_geom(p.window_h, p.window_w).len;
  a.vb = f.has_dv_bias;
  a.dt = f.has_dtable;
  // the fused 14 x 14 kernel has no v_bias-gradient output (the engine derives it from the proj dgrad: vit_engine.py);
  // given the forward output it computes delta itself
  if (o.attn16 && !f.has_dv_bias && attn16_fits(p)) {
    a.family = MEMHIP_ATTN_16;
    a.fd = f.has_out;
    a.nwg = nwg16(p, stream_cus);
    push(a, MEMHIP_ATTN_K_BWD16, a.nwg * p.heads, 1, 1, kAttn16ThreadsBwd, kAttn16LdsBwd);
    return a;
  }
  // every other family reads delta = rowsum(dout * out) from memory, and the per-head bounds of the table-gradient buckets
  // from `stats` (zeroed here, filled by the family's first kernel)
  if (f.has_out) push(a, MEMHIP_ATTN_K_DELTA, attn_delta_grid((int64_t)p.B * p.T, p.heads), 1, 1, 256, 0);
  if (f.has_dtable) push(a, MEMHIP_ATTN_K_STATS_ZERO, 1, 1, 1, 64, 0);
  if (nkb <= 8) {
    const int64_t sm_kv = (int64_t)4 * nkb * 32 * 128 + (int64_t)(glen + 6 * nkb * 32 + HD) * 4 + 32;
    const int64_t sm_q = (int64_t)4 * nkb * 32 * 128 + (int64_t)(2 * glen + HD + 2 * nkb * 32) * 4 + 32;
    if (!fits(sm_kv) || !fits(sm_q)) return over_budget(a, MEMHIP_ATTN_SMALL, sm_kv > sm_q ? sm_kv : sm_q);
    a.family = MEMHIP_ATTN_SMALL;
    a.n = nkb;
    a.spb = pick_spb(p, stream_cus);
    const int grid = cdiv(p.B, a.spb) * p.heads;
    push(a, MEMHIP_ATTN_K_BWD_KV, grid, 1, 1, 512, sm_kv);
    push(a, MEMHIP_ATTN_K_BWD_Q, grid, 1, 1, 512, sm_q);
    return a;
  }
  if (o.attn_win && attn_win_fits(p)) {
    const WinLds w = win_lds(p);
    a.nbz = win_slots(p.B, (long long)a.groups * p.heads, stream_cus);
    // Quirk kept: the kernel that owns the table gradient is persistent over at most 16 samples per workgroup (the
    // fixed-point bound of the buckets); the recomputing dQ kernel is launched on these slots with or without a table gradient
    a.nbq = a.nbz;
    while (cdiv(p.B, a.nbq) > 16) ++a.nbq;
    // the dS-storing form: attn_win == 1 only, the caller's workspace (memhip_attn_bwd_workspace bytes, 16-byte aligned),
    // and the LDS of its dK / dV kernel WITH the table gradient, whether or not this call has one
    if (o.attn_win == 1 && f.ws_ok && f.ws_bytes >= win_ws_need(p, TP) && fits(w.kvs)) {
      a.family = MEMHIP_ATTN_WIN_DS;
      a.ww = p.window_w;
      a.qs = win_qs(p);
      // max |dO_q|^2, max |delta_q| per head: a multiple of the head count (see the kernel), ~256 blocks
      if (f.has_dtable) push(a, MEMHIP_ATTN_K_WIN_STATS, p.heads * cdiv(256, p.heads), 1, 1, 256, 0);
      if (!f.has_dtable) a.nbq = a.nbz;      // here the dK / dV kernel owns the table gradient: capped only when there is one
      push(a, MEMHIP_ATTN_K_BWD_KVS_WIN, win_grid(p.heads, a.nbq, a.groups), 1, 1, 512, f.has_dtable ? w.kvs : w.kvs0);
      a.qgroups = cdiv(a.qs, 256);
      a.nbs = win_slots(p.B, (long long)a.qgroups * p.heads, stream_cus);
      push(a, MEMHIP_ATTN_K_BWD_QS_WIN, win_grid(p.heads, a.nbs, a.qgroups), 1, 1, 512, w.qs);
      return a;
    }
    if (fits(w.kv) && fits(w.q)) {
      a.family = MEMHIP_ATTN_WIN;
      a.ww = p.window_w;
      push(a, MEMHIP_ATTN_K_BWD_KV_WIN, win_grid(p.heads, a.nbz, a.groups), 1, 1, 512, w.kv);
      push(a, MEMHIP_ATTN_K_BWD_Q_WIN, win_grid(p.heads, a.nbq, a.groups), 1, 1, 512, w.q);
      return a;
    }
    a.nbz = a.nbq = 0;
  }
  constexpr int CTK = kKvCKB * 32, CTQ = kQCKB * 32;
  const int64_t sm_kv = (int64_t)4 * CTK * 128 + (int64_t)(glen + 2 * (cdiv(p.T, CTK) * CTK) + 4 * CTK + HD) * 4 + 32;
  const int64_t sm_q = (int64_t)4 * CTQ * 128 + (int64_t)(2 * glen + HD + 2 * (cdiv(p.T, CTQ) * CTQ)) * 4 + 32;
  if (!fits(sm_kv) || !fits(sm_q)) return over_budget(a, MEMHIP_ATTN_STREAM, sm_kv > sm_q ? sm_kv : sm_q);
  a.family = MEMHIP_ATTN_STREAM;
  push(a, MEMHIP_ATTN_K_BWD_KV_STREAM, a.groups, p.heads, p.B, 512, sm_kv);
  // samples per workgroup of the dQ kernel: amortise the bucket flush once the grid is a few rounds deep.
  // Quirk kept: one sample per 1024 workgroups of the one-sample grid, whatever the device; at most 16 (the buckets' bound)
  const long long spb = (long long)p.B * p.heads * a.groups / 1024;
  a.stream_spb = (int)(spb < 1 ? 1 : (spb > 16 ? 16 : spb));
  push(a, MEMHIP_ATTN_K_BWD_Q_STREAM, a.groups, p.heads, cdiv(p.B, a.stream_spb), 512, sm_q);
  return a;
}

}  // namespace memhip
