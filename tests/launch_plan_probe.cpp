// Prints what mvtracker_amd/csrc/launch_plan.h decides, for tests/test_launch_plan_host.py: one case per line of stdin, one line of
// stdout per case (`upd` prints one line per n of its range).  Host compiler only; no GPU, no HIP.
//
//   sw = nmb_forced nmb_force no_split time_small frame_small
//   block M H ws slices sw | time M S ws sw | partials M S H n_keys n_splits ws defer slices | frame M S H ws defer slices sw
//   ctx M S n_keys ws defer chunks next_N | input M | lnproj M slices | slices n N0 N1 N2
//   attn groups heads nq nk ws | partfloats G S heads | upd n_lo n_hi S G mask sw
//
// A plan prints as `ws=<uses_ws> bmv=<bmv> <NMB,MODE,ATT>(gx,gy,gz) ...`, or `refused`.
#include <stdio.h>
#include <string.h>

#include "../mvtracker_amd/csrc/launch_plan.h"

using namespace mvt_plan;

static bool read_ints(long long* v, int n) {
  for (int i = 0; i < n; ++i)
    if (scanf("%lld", &v[i]) != 1) return false;
  return true;
}

static BlockSwitches switches(const long long* v) { return BlockSwitches{(int)v[1], v[0] != 0, v[2] != 0, v[3] != 0, v[4] != 0}; }

static void print_plan(const BlockPlan& p) {
  if (!p.ok) {
    puts("refused");
    return;
  }
  printf("ws=%d bmv=%d", p.uses_ws ? 1 : 0, p.bmv);
  for (int i = 0; i < p.n; ++i) printf(" <%d,%d,%d>(%u,%u,%u)", p.l[i].nmb, p.l[i].mode, p.l[i].att, p.l[i].gx, p.l[i].gy, p.l[i].gz);
  putchar('\n');
}

static int key(const BlockPlan& p) { return p.ok ? p.l[0].nmb * 100 + p.l[0].mode * 10 + p.l[0].att : 0; }

int main() {
  static const char* const TIME[] = {"separate", "fused"};
  static const char* const V2P[] = {"plain", "partials", "segmented"};
  static const char* const VSELF[] = {"separate", "frame", "deferred", "segmented"};
  static const char* const P2V[] = {"separate", "frame", "ctx", "segmented"};
  static const char* const ATTN[] = {"keysplit", "ks4", "ks1"};
  char what[32];
  long long v[16];
  while (scanf("%31s", what) == 1) {
    bool ok = true;
    if (!strcmp(what, "block")) {
      if ((ok = read_ints(v, 9))) print_plan(plan_block(v[0], (int)v[1], v[2] != 0, (int)v[3], switches(v + 4)));
    } else if (!strcmp(what, "time")) {
      if ((ok = read_ints(v, 8))) print_plan(plan_time(v[0], (int)v[1], v[2] != 0, switches(v + 3)));
    } else if (!strcmp(what, "partials")) {
      if ((ok = read_ints(v, 8))) print_plan(plan_partials(v[0], (int)v[1], (int)v[2], (int)v[3], (int)v[4], v[5] != 0, v[6] != 0, (int)v[7]));
    } else if (!strcmp(what, "frame")) {
      if ((ok = read_ints(v, 11))) print_plan(plan_frame(v[0], (int)v[1], (int)v[2], v[3] != 0, v[4] != 0, (int)v[5], switches(v + 6)));
    } else if (!strcmp(what, "ctx")) {
      if ((ok = read_ints(v, 7))) print_plan(plan_frame_ctx(v[0], (int)v[1], (int)v[2], v[3] != 0, v[4] != 0, (int)v[5], (int)v[6]));
    } else if (!strcmp(what, "input")) {
      if ((ok = read_ints(v, 1))) print_plan(plan_input_proj(v[0]));
    } else if (!strcmp(what, "lnproj")) {
      if ((ok = read_ints(v, 2))) print_plan(plan_ln_proj(v[0], (int)v[1]));
    } else if (!strcmp(what, "slices")) {
      if ((ok = read_ints(v, 4))) {
        mvt_block_next nx[MVT_BLOCK_MAX_NEXT] = {};
        for (int q = 0; q < MVT_BLOCK_MAX_NEXT; ++q) nx[q].N = (int)v[1 + q];
        printf("%d\n", pass2_slices(nx, (int)v[0]));
      }
    } else if (!strcmp(what, "attn")) {
      if ((ok = read_ints(v, 5))) {
        const AttnForm f = attn_form(v[0], (int)v[1], (int)v[2], (int)v[3], v[4] != 0);
        printf("%s %lld\n", ATTN[f.kernel], f.blocks);
      }
    } else if (!strcmp(what, "partfloats")) {
      if ((ok = read_ints(v, 3))) printf("%lld\n", attn_partials_floats(v[0], v[1], (int)v[2]));
    } else if (!strcmp(what, "upd")) {
      if ((ok = read_ints(v, 10))) {
        const int S = (int)v[2], G = (int)v[3], mask = (int)v[4];
        const BlockSwitches sw = switches(v + 5);
        for (int n = (int)v[0]; n <= (int)v[1]; ++n) {
          const UpdaterForms f = updater_forms(n, S, G, mask, sw);
          const long long Mp = (long long)n * S, M = Mp + (long long)G * UPD_NV * S;
          // the first launch of the block entry that each in-kernel attention form calls, as updater.hip calls it
          const int tkey = f.time == TIME_FUSED ? key(plan_time(M, S, false, sw)) : 0;
          const int pkey = f.p2v == P2V_FRAME ? key(plan_frame(Mp, S, UPD_MLP, false, false, 1, sw))
                                              : (f.p2v == P2V_CTX ? key(plan_frame_ctx(Mp, S, UPD_NV, false, false, UPD_MLP / 256, 3 * UPD_INNER)) : 0);
          printf("%s %s %s %s %d %d\n", TIME[f.time], V2P[f.v2p], VSELF[f.vself], P2V[f.p2v], tkey, pkey);
        }
      }
    } else {
      ok = false;
    }
    if (!ok) {
      fprintf(stderr, "bad case: %s\n", what);
      return 2;
    }
  }
  return 0;
}
