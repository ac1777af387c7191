// Prints what mvtracker_amd/csrc/conv_plan.h decides, for tests/test_conv_plan_host.py: one case per line of stdin, one line of
// stdout per case.  Host compiler only; no GPU, no HIP.
//
//   sw = rows_nw8 conv_big fold_downsample
//   gemm M N | halo tiles N                                    -> tm tn wm wn blocks
//   fits tm tn ks s nw                                         -> patch_slots stage_elems fits
//   slots H W Cin KH KW stride pad split sw                    -> slots
//   conv n H W Cin Cout KH KW stride pad ldo act io fp32 lo in_stats out_partial in16 out16 w8 w16 lo8 stats16 sw
//   stem n H W Cout ldo io out16
//        -> family tm tn ks s nw inb staged split tile(tm tn wm wn) threads grid rows slots ldw, or `refused`
//   down n H W Cin Cout ldo same_partials al16                 -> tn threads grid rows slots ldw ldwd, or `refused`
//   enc n H W C sw  -> part_floats stat_channels fit, then per convolution H:W:Cin:Cout:k:stride:stats:with_down:folded:slots
#include <stdio.h>
#include <string.h>

#include "../mvtracker_amd/csrc/conv_plan.h"

using namespace mvt_plan;

static bool read_ints(long long* v, int n) {
  for (int i = 0; i < n; ++i)
    if (scanf("%lld", &v[i]) != 1) return false;
  return true;
}

static ConvSwitches switches(const long long* v) { return ConvSwitches{(int)v[0], v[1] != 0, v[2] != 0}; }

static void print_tile(const GemmTile& t) { printf("%d %d %d %d %lld\n", t.tm, t.tn, t.wm, t.wn, t.blocks); }

static void print_plan(const ConvPlan& p) {
  static const char* const FAMILY[] = {"refused", "gemm_f32", "im2col", "halo", "stem_rows", "rows", "big"};
  if (p.family == CONV_REFUSED) {
    puts("refused");
    return;
  }
  printf("%s %d %d %d %d %d %d %d %d %d %d %d %d %d %lld %d %d %d\n", FAMILY[p.family], p.tm, p.tn, p.ks, p.s, p.nw, p.inb ? 1 : 0, p.staged ? 1 : 0,
         p.split ? 1 : 0, p.tile.tm, p.tile.tn, p.tile.wm, p.tile.wn, p.threads, p.grid, p.rows, p.slots, p.ldw);
}

int main() {
  char what[32];
  long long v[32];
  while (scanf("%31s", what) == 1) {
    bool ok = true;
    if (!strcmp(what, "gemm")) {
      if ((ok = read_ints(v, 2))) print_tile(gemm_tile(v[0], (int)v[1]));
    } else if (!strcmp(what, "halo")) {
      if ((ok = read_ints(v, 2))) print_tile(halo_tile(v[0], (int)v[1]));
    } else if (!strcmp(what, "fits")) {
      if ((ok = read_ints(v, 5)))
        printf("%d %d %d\n", patch_slots((int)v[0], (int)v[2], (int)v[3], (int)v[4]), stage_elems((int)v[1]),
               rows_staged_fits((int)v[0], (int)v[1], (int)v[2], (int)v[3], (int)v[4]) ? 1 : 0);
    } else if (!strcmp(what, "slots")) {
      if ((ok = read_ints(v, 11)))
        printf("%d\n", conv_stat_slots((int)v[0], (int)v[1], (int)v[2], (int)v[3], (int)v[4], (int)v[5], (int)v[6], v[7] != 0, switches(v + 8)));
    } else if (!strcmp(what, "conv")) {
      if ((ok = read_ints(v, 25))) {
        ConvCall c{(int)v[0], (int)v[1], (int)v[2], (int)v[3], (int)v[4], (int)v[5], (int)v[6], (int)v[7], (int)v[8], (int)v[9], (int)v[10], (int)v[11]};
        c.fp32 = v[12] != 0, c.has_lo = v[13] != 0, c.has_in_stats = v[14] != 0, c.has_out_partial = v[15] != 0;
        c.in_al16 = v[16] != 0, c.out_al16 = v[17] != 0, c.w_al8 = v[18] != 0, c.w_al16 = v[19] != 0, c.lo_al8 = v[20] != 0, c.stats_al16 = v[21] != 0;
        print_plan(plan_conv(c, switches(v + 22)));
      }
    } else if (!strcmp(what, "stem")) {
      if ((ok = read_ints(v, 7))) print_plan(plan_stem((int)v[0], (int)v[1], (int)v[2], (int)v[3], (int)v[4], (int)v[5], v[6] != 0));
    } else if (!strcmp(what, "down")) {
      if ((ok = read_ints(v, 8))) {
        const DownPlan p = plan_down((int)v[0], (int)v[1], (int)v[2], (int)v[3], (int)v[4], (int)v[5], v[6] != 0, v[7] != 0);
        if (p.ok) printf("%d %d %lld %d %d %d %d\n", p.tn, p.threads, p.grid, p.rows, p.slots, p.ldw, p.ldwd);
        else puts("refused");
      }
    } else if (!strcmp(what, "enc")) {
      if ((ok = read_ints(v, 7))) {
        const ConvSwitches sw = switches(v + 4);
        EncConv t[MVT_ENCODER_CONVS];
        encoder_convs((int)v[1], (int)v[2], (int)v[3], sw, t);
        const long long pf = encoder_part_floats(v[0], (int)v[1], (int)v[2], (int)v[3]);
        printf("%lld %lld %d", pf, encoder_stat_channels((int)v[3]), encoder_partials_fit(t, v[0], pf, sw) ? 1 : 0);
        for (int i = 0; i < MVT_ENCODER_CONVS; ++i)
          printf(" %d:%d:%d:%d:%d:%d:%d:%d:%d:%d", t[i].H, t[i].W, t[i].Cin, t[i].Cout, t[i].k, t[i].stride, t[i].stats ? 1 : 0, t[i].with_down ? 1 : 0,
                 t[i].folded ? 1 : 0, encoder_slots(t[i], sw));
        putchar('\n');
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
