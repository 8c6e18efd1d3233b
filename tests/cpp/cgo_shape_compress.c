/* cgo_shape_compress.c — the compressed-form entry points of the C ABI used the way go/bgn_amd.go uses them, from plain
 * C (what cgo compiles): CompressBatch / DecompressBatch on host buffers and CompressBatchDev / DecompressBatchDev on
 * device arrays from bgn_dev_alloc on the null stream.  The elements and the expected compressed bytes come on the
 * command line as hex — the Python test computes them with Python integers; exit 0 iff every call returned the
 * expected bytes.  Compiled with `gcc -std=c99` by tests/test_cgo_shape_compress.py.
 *
 *   cgo_shape_compress P_HEX N_HEX L P_WIRE Q_WIRE  LEVEL FULL_HEX COMPRESSED_HEX
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
  uint8_t *p, *n, *Pw, *Qw, *full, *want, *comp, *back, *ok;
  void *d_full, *d_comp, *d_back, *d_ok;
  size_t p_len, n_len, E, CE, count, i;
  uint64_t l;
  bgn_ctx* ctx = NULL;
  int rc, level;
  if (argc != 9) {
    fprintf(stderr, "usage: see the header of cgo_shape_compress.c\n");
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
  CE = bgn_fp_bytes(ctx) + 1;
  level = atoi(argv[6]);
  count = unhex(argv[7], &full) / E;
  if (unhex(argv[8], &want) != count * CE) {
    fprintf(stderr, "the arrays do not fit COUNT = %zu\n", count);
    return 2;
  }
  comp = (uint8_t*)calloc(count, CE);
  back = (uint8_t*)calloc(count, E);
  ok = (uint8_t*)calloc(count, 1);

  /* e.CompressBatch, e.DecompressBatch (go/bgn_amd.go) */
  rc = bgn_compress_batch(ctx, count, level, full, comp);
  expect("CompressBatch", rc, comp, want, count * CE);
  rc = bgn_decompress_batch(ctx, count, level, want, back, ok);
  expect("DecompressBatch", rc, back, full, count * E);
  for (i = 0; i < count; ++i)
    if (ok[i] != 1) failures++;
  /* bad arguments are BGN_E_ARG, count 0 is BGN_OK */
  if (bgn_compress_batch(ctx, count, 3, full, comp) != BGN_E_ARG || bgn_compress_batch(ctx, count, level, NULL, comp) != BGN_E_ARG ||
      bgn_decompress_batch(ctx, count, level, want, back, NULL) != BGN_E_ARG ||
      bgn_compress_batch(NULL, count, level, full, comp) != BGN_E_ARG || bgn_compress_batch(ctx, 0, level, NULL, NULL) != BGN_OK ||
      bgn_decompress_batch(ctx, 0, level, NULL, NULL, NULL) != BGN_OK) {
    failures++;
    fprintf(stderr, "a bad argument was not refused with BGN_E_ARG\n");
  }

  /* e.CompressBatchDev, e.DecompressBatchDev: DeviceArrays on the null stream */
  d_full = bgn_dev_alloc(ctx, count * E);
  d_comp = bgn_dev_alloc(ctx, count * CE);
  d_back = bgn_dev_alloc(ctx, count * E);
  d_ok = bgn_dev_alloc(ctx, count);
  if (!d_full || !d_comp || !d_back || !d_ok) {
    fprintf(stderr, "bgn_dev_alloc failed: %s\n", bgn_last_error());
    return 4;
  }
  memset(comp, 0, count * CE);
  memset(back, 0, count * E);
  memset(ok, 0, count);
  rc = bgn_dev_upload(ctx, d_full, full, count * E);
  if (!rc) rc = bgn_compress_batch_dev(ctx, count, level, (const uint8_t*)d_full, (uint8_t*)d_comp, NULL);
  if (!rc) rc = bgn_dev_download(ctx, comp, d_comp, count * CE);
  expect("CompressBatchDev", rc, comp, want, count * CE);
  rc = bgn_decompress_batch_dev(ctx, count, level, (const uint8_t*)d_comp, (uint8_t*)d_back, (uint8_t*)d_ok, NULL);
  if (!rc) rc = bgn_dev_download(ctx, back, d_back, count * E);
  if (!rc) rc = bgn_dev_download(ctx, ok, d_ok, count);
  expect("DecompressBatchDev", rc, back, full, count * E);
  for (i = 0; i < count; ++i)
    if (ok[i] != 1) failures++;
  bgn_dev_free(ctx, d_full);
  bgn_dev_free(ctx, d_comp);
  bgn_dev_free(ctx, d_back);
  bgn_dev_free(ctx, d_ok);
  bgn_ctx_destroy(ctx);
  printf("cgo_shape_compress: %zu elements, %d failures\n", count, failures);
  return failures ? 1 : 0;
}
