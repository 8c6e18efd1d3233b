/* cgo_shape_sum.c — the segmented-sum entry points of the C ABI used the way go/bgn_amd.go uses them, from plain C (what
 * cgo compiles): SumBatch on host buffers (bgn_sum_batch) and SumBatchDev on device arrays from bgn_dev_alloc (the
 * shim's DeviceArray) on the null stream, deterministic and with one blinding scalar per segment.  The ciphertexts and
 * the expected sums come on the command line as hex — the Python test computes the sums with the oracle, from exponent
 * arithmetic; exit 0 iff every call returned the expected bytes.  Compiled with `gcc -std=c99` by
 * tests/test_cgo_shape_sum.py.
 *
 *   cgo_shape_sum P_HEX N_HEX L P_WIRE Q_WIRE  LEVEL SEG_LEN CT_HEX WANT_HEX  R_HEX WANT_BLINDED_HEX
 *
 * CT: NSEG * SEG_LEN elements; WANT, WANT_BLINDED: NSEG elements; R: NSEG rows of n_len bytes.
 */
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

static int failures;

static void expect(const char* what, int rc, const uint8_t* got, const uint8_t* want, size_t n) {
  if (rc || memcmp(got, want, n)) {
    failures++;
    fprintf(stderr, "%s failed (rc %d): %s\n", what, rc, rc ? bgn_last_error() : "bytes differ");
  }
}

int main(int argc, char** argv) {
  uint8_t *p, *n, *Pw, *Qw, *ct, *want, *r, *want_b, *out;
  void *d_ct, *d_r, *d_out;
  size_t p_len, n_len, E, nseg, seg_len, ct_bytes;
  uint64_t l;
  bgn_ctx* ctx = NULL;
  int rc, level;
  if (argc != 12) {
    fprintf(stderr, "usage: see the header of cgo_shape_sum.c\n");
    return 2;
  }
  p_len = unhex(argv[1], &p);
  n_len = unhex(argv[2], &n);
  l = strtoull(argv[3], NULL, 10);
  unhex(argv[4], &Pw);
  unhex(argv[5], &Qw);
  rc = bgn_ctx_create(&ctx, p, p_len, n, n_len, l, Pw, Qw, 1, 0);
  if (rc) {
    printf("bgn_ctx_create: %d %s\n", rc, bgn_last_error());
    return 3;
  }
  E = 2 * bgn_fp_bytes(ctx);
  level = atoi(argv[6]);
  seg_len = (size_t)strtoull(argv[7], NULL, 10);
  ct_bytes = unhex(argv[8], &ct);
  nseg = ct_bytes / E / seg_len;
  if (unhex(argv[9], &want) != nseg * E || unhex(argv[10], &r) != nseg * n_len || unhex(argv[11], &want_b) != nseg * E) {
    fprintf(stderr, "the arrays do not fit NSEG = %zu\n", nseg);
    return 2;
  }
  out = (uint8_t*)calloc(nseg, E);

  /* e.SumBatch (go/bgn_amd.go): deterministic, then with r */
  rc = bgn_sum_batch(ctx, nseg, seg_len, level, ct, NULL, 0, out);
  expect("SumBatch", rc, out, want, nseg * E);
  memset(out, 0, nseg * E);
  rc = bgn_sum_batch(ctx, nseg, seg_len, level, ct, r, n_len, out);
  expect("SumBatch with r", rc, out, want_b, nseg * E);
  /* bad arguments are BGN_E_ARG, nseg 0 is BGN_OK */
  if (bgn_sum_batch(ctx, nseg, 0, level, ct, NULL, 0, out) != BGN_E_ARG ||
      bgn_sum_batch(ctx, nseg, seg_len, 3, ct, NULL, 0, out) != BGN_E_ARG ||
      bgn_sum_batch(ctx, nseg, seg_len, level, NULL, NULL, 0, out) != BGN_E_ARG ||
      bgn_sum_batch(NULL, nseg, seg_len, level, ct, NULL, 0, out) != BGN_E_ARG ||
      bgn_sum_batch(ctx, 0, seg_len, level, ct, NULL, 0, out) != BGN_OK) {
    failures++;
    fprintf(stderr, "a bad argument was not refused with BGN_E_ARG\n");
  }

  /* e.SumBatchDev: DeviceArrays on the null stream */
  d_ct = bgn_dev_alloc(ctx, ct_bytes);
  d_r = bgn_dev_alloc(ctx, nseg * n_len);
  d_out = bgn_dev_alloc(ctx, nseg * E);
  if (!d_ct || !d_r || !d_out) {
    fprintf(stderr, "bgn_dev_alloc failed: %s\n", bgn_last_error());
    return 4;
  }
  memset(out, 0, nseg * E);
  rc = bgn_dev_upload(ctx, d_ct, ct, ct_bytes);
  if (!rc) rc = bgn_dev_upload(ctx, d_r, r, nseg * n_len);
  if (!rc) rc = bgn_sum_batch_dev(ctx, nseg, seg_len, level, (const uint8_t*)d_ct, NULL, 0, (uint8_t*)d_out, NULL);
  if (!rc) rc = bgn_dev_download(ctx, out, d_out, nseg * E);
  expect("SumBatchDev", rc, out, want, nseg * E);
  memset(out, 0, nseg * E);
  rc = bgn_sum_batch_dev(ctx, nseg, seg_len, level, (const uint8_t*)d_ct, (const uint8_t*)d_r, n_len, (uint8_t*)d_out, NULL);
  if (!rc) rc = bgn_dev_download(ctx, out, d_out, nseg * E);
  expect("SumBatchDev with r", rc, out, want_b, nseg * E);
  bgn_dev_free(ctx, d_ct);
  bgn_dev_free(ctx, d_r);
  bgn_dev_free(ctx, d_out);
  bgn_ctx_destroy(ctx);
  printf("cgo_shape_sum: %zu sums, %d failures\n", nseg, failures);
  return failures ? 1 : 0;
}
