/* cgo_shape_scan.c — bgn_scan_batch and bgn_scan_batch_dev used the way go/bgn_amd.go's ScanBatch and ScanBatchDev use
 * them, from plain C (what cgo compiles), deterministic and blinded.  Exit 0 iff every call returned the expected bytes,
 * which tests/test_cgo_shape_scan.py computes with the oracle and hands in as hex:
 *   cgo_shape_scan P_HEX N_HEX L P_WIRE Q_WIRE  LEVEL SEG_LEN CT_HEX WANT_HEX  R_HEX WANT_BLINDED_HEX */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "bgn_amd.h"

static size_t unhex(const char* s, uint8_t** out) {
  size_t n = strlen(s) / 2, i;
  *out = (uint8_t*)malloc(n ? n : 1);
  for (i = 0; i < n; ++i) {
    unsigned v;
    sscanf(s + 2 * i, "%2x", &v);
    (*out)[i] = (uint8_t)v;
  }
  return n;
}

int main(int argc, char** argv) {
  uint8_t *p, *n, *Pw, *Qw, *ct, *want[2], *r, *out;
  void *d_ct, *d_r, *d_out;
  size_t p_len, n_len, E, nseg, seg_len, nb;
  bgn_ctx* ctx = NULL;
  int rc, level, blind, failures = 0;
  if (argc != 12) return 2;
  p_len = unhex(argv[1], &p);
  n_len = unhex(argv[2], &n);
  unhex(argv[4], &Pw);
  unhex(argv[5], &Qw);
  rc = bgn_ctx_create(&ctx, p, p_len, n, n_len, strtoull(argv[3], NULL, 10), Pw, Qw, 1, 0);
  if (rc) {
    printf("bgn_ctx_create: %d %s\n", rc, bgn_last_error());
    return 3;
  }
  E = 2 * bgn_fp_bytes(ctx);
  level = atoi(argv[6]);
  seg_len = (size_t)strtoull(argv[7], NULL, 10);
  nb = unhex(argv[8], &ct);
  nseg = nb / E / seg_len;
  if (unhex(argv[9], &want[0]) != nb || unhex(argv[10], &r) != nb / E * n_len || unhex(argv[11], &want[1]) != nb) return 2;
  out = (uint8_t*)malloc(nb);
  d_ct = bgn_dev_alloc(ctx, nb);
  d_r = bgn_dev_alloc(ctx, nb / E * n_len);
  d_out = bgn_dev_alloc(ctx, nb);
  if (!d_ct || !d_r || !d_out || bgn_dev_upload(ctx, d_ct, ct, nb) || bgn_dev_upload(ctx, d_r, r, nb / E * n_len)) return 4;
  for (blind = 0; blind < 2; ++blind) {
    memset(out, 0, nb);
    rc = bgn_scan_batch(ctx, nseg, seg_len, level, ct, blind ? r : NULL, blind ? n_len : 0, out);
    if (rc || memcmp(out, want[blind], nb)) failures++;
    memset(out, 0, nb);
    rc = bgn_scan_batch_dev(ctx, nseg, seg_len, level, (const uint8_t*)d_ct, blind ? (const uint8_t*)d_r : NULL,
                            blind ? n_len : 0, (uint8_t*)d_out, NULL);
    if (!rc) rc = bgn_dev_download(ctx, out, d_out, nb);
    if (rc || memcmp(out, want[blind], nb)) failures++;
  }
  /* behind the null-context check: refused on a live context too */
  if (bgn_scan_batch(ctx, nseg, 0, level, ct, NULL, 0, out) != BGN_E_ARG || bgn_scan_batch(ctx, nseg, seg_len, 3, ct, NULL, 0, out) != BGN_E_ARG ||
      bgn_scan_batch(ctx, nseg, seg_len, level, NULL, NULL, 0, out) != BGN_E_ARG || bgn_scan_batch(ctx, nseg, seg_len, level, ct, r, 0, out) != BGN_E_ARG)
    failures++;
  bgn_dev_free(ctx, d_ct);
  bgn_dev_free(ctx, d_r);
  bgn_dev_free(ctx, d_out);
  bgn_ctx_destroy(ctx);
  printf("cgo_shape_scan: %zu prefixes, %d failures\n", nb / E, failures);
  return failures ? 1 : 0;
}
