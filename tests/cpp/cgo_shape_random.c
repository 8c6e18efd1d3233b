/* cgo_shape_random.c — the seeded-randomness entry points of the C ABI used the way go/bgn_amd.go uses them, from plain
 * C (what cgo compiles): every new call of the Go shim has its twin here.  Host buffers: bgn_random_scalars_batch,
 * bgn_encrypt_seeded_batch; device arrays from bgn_dev_alloc (the shim's DeviceArray): the `_dev` forms on the null
 * stream, the seed a host pointer; two contexts on device 0: bgn_mencrypt_seeded_batch.  The expected rows come on the
 * command line as hex — the Python test computes them with hashlib and integers — and the expected ciphertexts are
 * bgn_encrypt_batch of those rows; exit 0 iff every call returned the expected bytes.  Compiled with `gcc -std=c99` by
 * tests/test_cgo_shape_random.py.
 *
 *   cgo_shape_random P_HEX N_HEX L P_WIRE Q_WIRE  SEED_HEX STREAM_ID FIRST_INDEX X_HEX  WANT_R
 *
 * X: COUNT plaintexts of 8 bytes each, back to back; WANT_R: COUNT rows of n_len bytes.
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
  uint8_t *p, *n, *Pw, *Qw, *seed, *x, *want_r, *want_ct, *r, *ct;
  void *d_x, *d_r, *d_ct;
  size_t p_len, n_len, E, count;
  const size_t x_len = 8;
  uint64_t stream_id, first, l;
  bgn_ctx* ctx = NULL;
  bgn_mctx* mctx = NULL;
  const int devices[2] = {0, 0};
  int rc;
  if (argc != 11) {
    fprintf(stderr, "usage: see the header of cgo_shape_random.c\n");
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
  if (unhex(argv[6], &seed) != 32) {
    fprintf(stderr, "the seed is 32 bytes\n");
    return 2;
  }
  stream_id = strtoull(argv[7], NULL, 10);
  first = strtoull(argv[8], NULL, 10);
  count = unhex(argv[9], &x) / x_len;
  unhex(argv[10], &want_r);
  r = (uint8_t*)calloc(count, n_len);
  ct = (uint8_t*)calloc(count, E);
  want_ct = (uint8_t*)calloc(count, E);
  rc = bgn_encrypt_batch(ctx, count, x, x_len, want_r, n_len, want_ct);
  if (rc) {
    fprintf(stderr, "bgn_encrypt_batch: %d %s\n", rc, bgn_last_error());
    return 4;
  }

  /* pk.RandomScalars, pk.EncryptBatchSeeded (go/bgn_amd.go) */
  rc = bgn_random_scalars_batch(ctx, count, seed, stream_id, first, r);
  expect("RandomScalars", rc, r, want_r, count * n_len);
  rc = bgn_encrypt_seeded_batch(ctx, count, x, x_len, seed, stream_id, first, ct);
  expect("EncryptBatchSeeded", rc, ct, want_ct, count * E);
  /* bad arguments are BGN_E_ARG, count 0 is BGN_OK */
  if (bgn_random_scalars_batch(ctx, count, NULL, stream_id, first, r) != BGN_E_ARG ||
      bgn_random_scalars_batch(ctx, 2, seed, stream_id, UINT64_MAX, r) != BGN_E_ARG ||
      bgn_encrypt_seeded_batch(ctx, count, x, 0, seed, stream_id, first, ct) != BGN_E_ARG ||
      bgn_encrypt_seeded_batch(NULL, count, x, x_len, seed, stream_id, first, ct) != BGN_E_ARG ||
      bgn_encrypt_seeded_batch(ctx, 0, x, x_len, seed, stream_id, first, ct) != BGN_OK) {
    failures++;
    fprintf(stderr, "a bad argument was not refused with BGN_E_ARG\n");
  }

  /* DeviceArray forms: RandomScalarsDev, EncryptSeededDev on the null stream */
  d_x = bgn_dev_alloc(ctx, count * x_len);
  d_r = bgn_dev_alloc(ctx, count * n_len);
  d_ct = bgn_dev_alloc(ctx, count * E);
  if (!d_x || !d_r || !d_ct) {
    fprintf(stderr, "bgn_dev_alloc failed: %s\n", bgn_last_error());
    return 4;
  }
  memset(r, 0, count * n_len);
  memset(ct, 0, count * E);
  rc = bgn_dev_upload(ctx, d_x, x, count * x_len);
  if (!rc) rc = bgn_random_scalars_batch_dev(ctx, count, seed, stream_id, first, (uint8_t*)d_r, NULL);
  if (!rc) rc = bgn_encrypt_seeded_batch_dev(ctx, count, (const uint8_t*)d_x, x_len, seed, stream_id, first, (uint8_t*)d_ct, NULL);
  if (!rc) rc = bgn_dev_download(ctx, r, d_r, count * n_len);
  if (!rc) rc = bgn_dev_download(ctx, ct, d_ct, count * E);
  expect("RandomScalarsDev", rc, r, want_r, count * n_len);
  expect("EncryptSeededDev", rc, ct, want_ct, count * E);
  /* the rows as r of the existing Encrypt: what a caller does for Add / Mult / MultConst */
  memset(ct, 0, count * E);
  rc = bgn_encrypt_batch_dev(ctx, count, (const uint8_t*)d_x, x_len, (const uint8_t*)d_r, n_len, (uint8_t*)d_ct, NULL);
  if (!rc) rc = bgn_dev_download(ctx, ct, d_ct, count * E);
  expect("EncryptDev with the rows", rc, ct, want_ct, count * E);
  bgn_dev_free(ctx, d_x);
  bgn_dev_free(ctx, d_r);
  bgn_dev_free(ctx, d_ct);

  /* MultiPublicKey.EncryptBatchSeeded: two contexts on device 0 */
  rc = bgn_mctx_create(&mctx, p, p_len, n, n_len, l, Pw, Qw, 1, devices, 2);
  if (rc) {
    failures++;
    fprintf(stderr, "bgn_mctx_create: %d %s\n", rc, bgn_last_error());
  } else {
    memset(ct, 0, count * E);
    rc = bgn_mencrypt_seeded_batch(mctx, count, x, x_len, seed, stream_id, first, ct);
    expect("Multi EncryptBatchSeeded", rc, ct, want_ct, count * E);
    if (bgn_mencrypt_seeded_batch(mctx, count, x, x_len, NULL, stream_id, first, ct) != BGN_E_ARG) {
      failures++;
      fprintf(stderr, "a null seed was not refused with BGN_E_ARG\n");
    }
    bgn_mctx_destroy(mctx);
  }
  bgn_ctx_destroy(ctx);
  printf("cgo_shape_random: %zu rows, %d failures\n", count, failures);
  return failures ? 1 : 0;
}
