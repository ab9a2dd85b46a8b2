/*
 * hsfft_schedule.c -- Stockham pass scheduling of libhsfft.so (host C): the effective stage list
 * of the reference recursion, its grouping into passes with their tiles and kernel variants, and
 * the odd-radix constants.  hs_build_schedule is the one entry point (hsfft_exec.c: entry_build).
 */
#define _GNU_SOURCE
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "hsfft_host.h"

/* Effective stage list of the reference recursion: descend with data_length = M taking
 * factors[fi]; a data_length in {2,3,4,5,7,8} is a leaf butterfly of that size (ref
 * :332-713 dispatch on data_length before radix).  Returns stages innermost first. */
static int effective_stages(int M, const int *fac, int lf, int *out, int *first_leaf)
{
    int outer[HS_MAX_STAGES], n = 0, len = M, fi = 0;
    *first_leaf = 0;
    while (len > 1) {
        if (hs_is_leaf_radix(len)) {
            outer[n++] = len;
            *first_leaf = 1;
            break;
        }
        if (fi >= lf || fac[fi] <= 1 || len % fac[fi] != 0 || n >= HS_MAX_STAGES) return -1;
        outer[n++] = fac[fi];
        len /= fac[fi++];
    }
    for (int i = 0; i < n; i++) out[i] = outer[n - 1 - i];
    return n;
}

static int pass_pmax(void)
{
    const int v = hs_env_int("HSFFT_PMAX", 512);
    return v < 8 ? 8 : v;
}

/* Register-kernel schedule for radix lists [r0, 8, 8, ...] (r0 in {2,4,8}; hsfft_pass_r8.h):
 * first pass [r0, 8^k1] with P <= 2048, then passes of 8^k (k <= 3), as few passes as
 * possible and as even as possible.  Tiles come from the variant table of the kernel. */
static int build_passes_pow2(hs_entry *e)
{
    const int r0 = e->stage_r[0];
    if (!e->first_leaf || !(r0 == 2 || r0 == 4 || r0 == 8)) return -1;
    for (int s = 1; s < e->nst; s++)
        if (e->stage_r[s] != 8) return -1;
    if (hs_env_int("HSFFT_GENERIC", 0)) return -1;
    int n8 = e->nst - 1;            /* radix-8 stages after stage 0 */
    /* at most 4 stages per pass; P <= 2048 unless r0 == 8 and a 4096-point first pass
     * saves a whole pass (2^21 = [8,8,8,8] + [8,8,8]) */
    int k1max = r0 == 8 ? (n8 == 6 ? 3 : 2) : 3;
    /* the whole transform as ONE pass when it fits one workgroup (P <= 8192 points, <= 1024
     * threads of 8 points): one HBM round trip instead of two -- 4096 = [8,8,8,8] and
     * 8192 = [2,8,8,8,8] (HSFFT_WHOLE=0: the two-pass schedule) */
    {
        long long pall = r0;
        for (int i = 0; i < n8; i++) pall *= 8;
        if (n8 <= 4 && pall <= 8192 && hs_env_int("HSFFT_WHOLE", 1) && r8_has_variant(r0, n8, 1, 1, 1)) k1max = n8;
    }
    /* number of later passes needed if the first takes k1 eights: ceil((n8-k1)/3) */
    int best_k1 = -1, best_np = 1 << 30, best_bal = 1 << 30;
    for (int k1 = r0 == 8 ? 0 : 1; k1 <= k1max && k1 <= n8; k1++) { /* every pass needs P >= 8 */
        const int rest = n8 - k1, np = 1 + (rest + 2) / 3;
        int bal = 0;
        if (rest) {
            const int per = (rest + (np - 1) - 1) / (np - 1);
            bal = per > k1 + 1 ? per - k1 - 1 : k1 + 1 - per;
        }
        const int forced = hs_env_int("HSFFT_K1", -1);
        if (forced >= 0 && k1 != forced) continue;
        if (np < best_np || (np == best_np && bal < best_bal)) {
            best_np = np;
            best_bal = bal;
            best_k1 = k1;
        }
    }
    if (best_k1 < 0 || best_np > HS_MAX_PASSES) return -1;
    long long B = 1;
    int np = 0, s = 0;
    const int later = best_np - 1;
    int remaining = n8 - best_k1;
    for (int ip = 0; ip < best_np; ip++) {
        hsd_pass *p = &e->pass[np++];
        memset(p, 0, sizeof *p);
        int k = ip == 0 ? best_k1 : (remaining + (later - (ip - 1)) - 1) / (later - (ip - 1));
        if (ip > 0) remaining -= k;
        p->nst = ip == 0 ? 1 + k : k;
        p->P = 1;
        for (int i = 0; i < p->nst; i++) {
            p->radix[i] = e->stage_r[s++];
            p->gcs_off[i] = -1;
            p->P *= p->radix[i];
        }
        p->leaf = ip == 0;
        p->B = B;
        p->A = e->M / (B * p->P);
        p->variant = HS_KV_R8X3;
        if (ip == 0) {
            /* WM columns per workgroup: as many as the LDS (<=128 KiB) and the variant table allow */
            static const int gopts[] = {32, 16, 8, 4, 2, 1};
            int gmax = hs_env_int("HSFFT_G1", 0);
            if (gmax <= 0) gmax = p->P >= 4096 ? 1 : p->P >= 2048 ? 2 : p->P >= 1024 ? 4 : p->P >= 512 ? 8 : p->P >= 64 ? 16 : 32;
            int G = 1;
            for (unsigned i = 0; i < sizeof gopts / sizeof gopts[0]; i++)
                if (gopts[i] <= gmax && gopts[i] <= p->A && r8_has_variant(p->radix[0], p->nst - 1, gopts[i], 1, 1)) {
                    G = gopts[i];
                    break;
                }
            p->Wm = G;
            p->Wq = 1;
            p->G = G;
        } else {
            static const int gopts[] = {32, 16, 8, 4};
            int gmax = hs_env_int("HSFFT_G2", 0);
            if (gmax <= 0) gmax = p->P >= 512 ? 8 : 32;
            int G = 0;
            for (unsigned i = 0; i < sizeof gopts / sizeof gopts[0]; i++)
                if (gopts[i] <= gmax && gopts[i] <= B && r8_has_variant(8, p->nst - 1, gopts[i], gopts[i], 0)) {
                    G = gopts[i];
                    break;
                }
            if (!G) return -1;
            p->Wm = 1;
            p->Wq = G;
            p->G = G;
        }
        B *= p->P;
    }
    e->npass = np;
    return 0;
}

/* Groups stages into passes of at most Pmax points and chooses the tile so that global
 * loads/stores move >= 128 contiguous bytes (8 complex) per row where the shape allows. */
static int build_passes(hs_entry *e)
{
    if (build_passes_pow2(e) == 0) return 0;
    if (e->nst <= HS_MAX_PASS_STAGES && hs_env_int("HSFFT_MR_ROW", 1) && !hs_env_int("HSFFT_GENERIC", 0)) {
        /* a whole-row kernel for this radix list (hsfft_pass_mr.h k_row): one pass, one HBM
         * round trip per row */
        hsd_pass *p = &e->pass[0];
        memset(p, 0, sizeof *p);
        p->nst = e->nst;
        p->P = 1;
        for (int s = 0; s < e->nst; s++) {
            p->radix[s] = e->stage_r[s];
            p->gcs_off[s] = -1;
            p->P *= e->stage_r[s];
        }
        p->leaf = e->first_leaf;
        p->B = 1;
        p->A = 1;
        p->Wq = p->Wm = p->G = 1;
        p->variant = HS_KV_MR;
        if (p->P == e->M && mr_has_variant(p)) {
            e->npass = 1;
            return 0;
        }
    }
    /* a whole row that fits the generic kernel's LDS ping-pong (32 B per point <= 160 KiB):
     * one pass, one HBM round trip, instead of passes of <= Pmax points (HSFFT_WHOLE=0) */
    int odd = 0, nodd = 0; /* distinct odd radices >= 11 (the generic kernel specialises one) */
    for (int i = 0; i < e->nst; i++) {
        const int r = e->stage_r[i];
        if (hs_is_leaf_radix(r) || r == odd) continue;
        odd = r;
        nodd++;
    }
    const int whole = hs_env_int("HSFFT_WHOLE", 1) && e->M <= 5120 && e->nst <= HS_MAX_PASS_STAGES && nodd <= 1;
    const int pmax = whole ? e->M : pass_pmax();
    int s = 0, np = 0;
    long long B = 1;
    while (s < e->nst) {
        if (np >= HS_MAX_PASSES) return -1;
        hsd_pass *p = &e->pass[np];
        memset(p, 0, sizeof *p);
        p->P = 1;
        p->leaf = (s == 0) && e->first_leaf;
        while (s < e->nst && p->nst < HS_MAX_PASS_STAGES && (p->nst == 0 || (long long)p->P * e->stage_r[s] <= pmax)) {
            p->radix[p->nst] = e->stage_r[s];
            p->gcs_off[p->nst] = -1;
            p->P *= e->stage_r[s];
            p->nst++;
            s++;
        }
        p->B = B;
        p->A = e->M / (B * p->P);
        int gmax = 2048 / p->P;
        if (gmax < 1) gmax = 1;
        int wq = (int)(B < 8 ? B : 8);
        if (wq > gmax) wq = gmax;
        int wm = 8 / wq;
        if (wm * wq > gmax) wm = gmax / wq;
        if (wm < 1) wm = 1;
        if (wm > p->A) wm = (int)p->A;
        p->Wq = wq;
        p->Wm = wm;
        p->G = wq * wm;
        p->variant = HS_KV_GENERIC;
        if (!hs_env_int("HSFFT_GENERIC", 0) && mr_has_variant(p)) p->variant = HS_KV_MR;
        B *= p->P;
        np++;
    }
    e->npass = np;
    return 0;
}

/* odd-radix constants: cos/sin(i*PI2/p) for i <= (p-1)/2, mirrored (ref :1527-1541) */
static int build_gcs(hs_entry *e)
{
    int total = 0;
    for (int i = 0; i < e->npass; i++)
        for (int s = 0; s < e->pass[i].nst; s++) {
            int r = e->pass[i].radix[s];
            if (hs_is_leaf_radix(r)) continue;
            if (r > 63) {
                hs_seterr("radix %d exceeds the odd-radix kernel limit (63)", r);
                return -1;
            }
            total += 2 * (r - 1);
        }
    e->ngcs = total;
    e->gcs = total ? malloc(sizeof(double) * (size_t)total) : NULL;
    int off = 0;
    for (int i = 0; i < e->npass; i++)
        for (int s = 0; s < e->pass[i].nst; s++) {
            int r = e->pass[i].radix[s];
            if (hs_is_leaf_radix(r)) continue;
            const int mid = (r - 1) / 2;
            double *cs = e->gcs + off, *sn = cs + (r - 1);
            for (int k = 1; k <= mid; k++) {
                double sv, cv;
                sincos(k * PI2 / r, &sv, &cv);
                cs[k - 1] = cv;
                sn[k - 1] = sv;
            }
            for (int k = 0; k < mid; k++) {
                sn[k + mid] = -sn[mid - 1 - k];
                cs[k + mid] = cs[mid - 1 - k];
            }
            e->pass[i].gcs_off[s] = off;
            off += 2 * (r - 1);
        }
    return 0;
}

/* the schedule of e->M = the product of e->rfac (M > 1): stages, passes, odd-radix constants */
int hs_build_schedule(hs_entry *e)
{
    e->nst = effective_stages(e->M, e->rfac, e->rlf, e->stage_r, &e->first_leaf);
    if (e->nst < 0) {
        hs_seterr("factor list of the plan does not describe length %d", e->M);
        return -1;
    }
    if (build_passes(e) || build_gcs(e)) return -1;
    if (hs_env_int("HSFFT_PLAN_DEBUG", 0)) { /* dev: the pass schedule */
        fprintf(stderr, "hsfft plan N=%d M=%d:", e->N, e->M);
        for (int i = 0; i < e->npass; i++) {
            const hsd_pass *p = &e->pass[i];
            fprintf(stderr, " [P=%d r=", p->P);
            for (int s = 0; s < p->nst; s++) fprintf(stderr, "%s%d", s ? "," : "", p->radix[s]);
            fprintf(stderr, " A=%lld B=%lld G=%d Wq=%d v=%d]", (long long)p->A, (long long)p->B, p->G, p->Wq, p->variant);
        }
        fprintf(stderr, "\n");
    }
    return 0;
}
