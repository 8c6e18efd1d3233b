/* cgo_shape_proofs.c — the proof entry points of the C ABI used the way go/bgn_amd.go uses them, from plain C (what cgo
 * compiles): every new call of the Go shim has its twin here.  Host buffers: bgn_prove_plaintext_knowledge_batch,
 * bgn_challenge_batch, bgn_verify_plaintext_knowledge_batch.  Device arrays from bgn_dev_alloc (the shim's DeviceArray):
 * the same three through their `_dev` forms on the null stream, with only the verdicts downloaded.  Inputs and the
 * expected proof come on the command line as hex (the Python test computes them with the host mirror); exit 0 iff every
 * call returned the expected bytes.  Compiled with `gcc -std=c99` by tests/test_cgo_shape_proofs.py.
 *
 *   cgo_shape_proofs P_HEX N_HEX L P_WIRE Q_WIRE  V_HEX Z_HEX NONCE1_HEX RQ_HEX  WANT_CT WANT_NONCE WANT_DL WANT_C
 *
 * V, Z, NONCE1: COUNT scalars of n_len bytes each, back to back; RQ: n_len bytes.
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
  uint8_t *p, *n, *Pw, *Qw, *v, *z, *a, *rq, *want_ct, *want_nonce, *want_dl, *want_c;
  uint8_t *ct, *nonce, *dl, *c, *ok;
  void *d_v, *d_z, *d_a, *d_rq, *d_ct, *d_nonce, *d_dl, *d_c, *d_ok;
  size_t p_len, n_len, E, count, i;
  bgn_ctx* ctx = NULL;
  int rc;
  if (argc != 14) {
    fprintf(stderr, "usage: see the header of cgo_shape_proofs.c\n");
    return 2;
  }
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
  count = unhex(argv[6], &v) / n_len;
  unhex(argv[7], &z);
  unhex(argv[8], &a);
  unhex(argv[9], &rq);
  unhex(argv[10], &want_ct);
  unhex(argv[11], &want_nonce);
  unhex(argv[12], &want_dl);
  unhex(argv[13], &want_c);
  ct = (uint8_t*)calloc(count, E);
  nonce = (uint8_t*)calloc(count, E);
  dl = (uint8_t*)calloc(count, n_len);
  c = (uint8_t*)calloc(count, 32);
  ok = (uint8_t*)calloc(count, 1);

  /* pk.NewProofOfPlaintextKnowledgeBatch, pk.ChallengeBatch, pk.CheckProofOfPlaintextKnoewledgeBatch (go/bgn_amd.go) */
  rc = bgn_prove_plaintext_knowledge_batch(ctx, count, v, n_len, z, n_len, a, n_len, rq, n_len, ct, nonce, dl);
  expect("Prove ct", rc, ct, want_ct, count * E);
  expect("Prove nonce", rc, nonce, want_nonce, count * E);
  expect("Prove dl", rc, dl, want_dl, count * n_len);
  rc = bgn_challenge_batch(ctx, count, ct, nonce, c);
  expect("Challenge", rc, c, want_c, count * 32);
  rc = bgn_verify_plaintext_knowledge_batch(ctx, count, ct, ct, nonce, dl, n_len, ok);
  for (i = 0; i < count; ++i)
    if (rc || ok[i] != 1) {
      failures++;
      fprintf(stderr, "Verify: proof %zu rejected (rc %d)\n", i, rc);
    }
  /* a proof of another ciphertext is rejected: the first ciphertext under test replaced by the second */
  if (count >= 2) {
    uint8_t* other = (uint8_t*)malloc(count * E);
    memcpy(other, ct, count * E);
    memcpy(other, ct + E, E);
    rc = bgn_verify_plaintext_knowledge_batch(ctx, count, other, ct, nonce, dl, n_len, ok);
    if (rc || ok[0] != 0 || ok[1] != 1) {
      failures++;
      fprintf(stderr, "Verify: wrong verdicts for a swapped ciphertext (rc %d, %d %d)\n", rc, ok[0], ok[1]);
    }
    free(other);
  }
  /* bad arguments are BGN_E_ARG */
  if (bgn_prove_plaintext_knowledge_batch(ctx, count, v, n_len + 1, z, n_len, a, n_len, rq, n_len, ct, nonce, dl) != BGN_E_ARG ||
      bgn_prove_plaintext_knowledge_batch(ctx, count, v, n_len, z, n_len, a, n_len, rq, 0, ct, nonce, dl) != BGN_E_ARG ||
      bgn_challenge_batch(ctx, count, ct, NULL, c) != BGN_E_ARG ||
      bgn_verify_plaintext_knowledge_batch(NULL, count, ct, ct, nonce, dl, n_len, ok) != BGN_E_ARG) {
    failures++;
    fprintf(stderr, "a bad argument was not refused with BGN_E_ARG\n");
  }

  /* DeviceArray forms: ProveDev, ChallengeDev, VerifyDev on the null stream */
  d_v = bgn_dev_alloc(ctx, count * n_len);
  d_z = bgn_dev_alloc(ctx, count * n_len);
  d_a = bgn_dev_alloc(ctx, count * n_len);
  d_rq = bgn_dev_alloc(ctx, n_len);
  d_ct = bgn_dev_alloc(ctx, count * E);
  d_nonce = bgn_dev_alloc(ctx, count * E);
  d_dl = bgn_dev_alloc(ctx, count * n_len);
  d_c = bgn_dev_alloc(ctx, count * 32);
  d_ok = bgn_dev_alloc(ctx, count);
  if (!d_v || !d_z || !d_a || !d_rq || !d_ct || !d_nonce || !d_dl || !d_c || !d_ok) {
    fprintf(stderr, "bgn_dev_alloc failed: %s\n", bgn_last_error());
    return 4;
  }
  rc = bgn_dev_upload(ctx, d_v, v, count * n_len);
  if (!rc) rc = bgn_dev_upload(ctx, d_z, z, count * n_len);
  if (!rc) rc = bgn_dev_upload(ctx, d_a, a, count * n_len);
  if (!rc) rc = bgn_dev_upload(ctx, d_rq, rq, n_len);
  if (!rc)
    rc = bgn_prove_plaintext_knowledge_batch_dev(ctx, count, (const uint8_t*)d_v, n_len, (const uint8_t*)d_z, n_len,
                                                 (const uint8_t*)d_a, n_len, (const uint8_t*)d_rq, n_len, (uint8_t*)d_ct,
                                                 (uint8_t*)d_nonce, (uint8_t*)d_dl, NULL);
  if (!rc) rc = bgn_challenge_batch_dev(ctx, count, (const uint8_t*)d_ct, (const uint8_t*)d_nonce, (uint8_t*)d_c, NULL);
  if (!rc)
    rc = bgn_verify_plaintext_knowledge_batch_dev(ctx, count, (const uint8_t*)d_ct, (const uint8_t*)d_ct,
                                                  (const uint8_t*)d_nonce, (const uint8_t*)d_dl, n_len, (uint8_t*)d_ok, NULL);
  memset(ct, 0, count * E);
  memset(dl, 0, count * n_len);
  memset(c, 0, count * 32);
  memset(ok, 0, count);
  if (!rc) rc = bgn_dev_download(ctx, ct, d_ct, count * E);
  if (!rc) rc = bgn_dev_download(ctx, dl, d_dl, count * n_len);
  if (!rc) rc = bgn_dev_download(ctx, c, d_c, count * 32);
  if (!rc) rc = bgn_dev_download(ctx, ok, d_ok, count);
  expect("ProveDev ct", rc, ct, want_ct, count * E);
  expect("ProveDev dl", rc, dl, want_dl, count * n_len);
  expect("ChallengeDev", rc, c, want_c, count * 32);
  for (i = 0; i < count; ++i)
    if (rc || ok[i] != 1) {
      failures++;
      fprintf(stderr, "VerifyDev: proof %zu rejected (rc %d)\n", i, rc);
    }
  bgn_dev_free(ctx, d_v);
  bgn_dev_free(ctx, d_z);
  bgn_dev_free(ctx, d_a);
  bgn_dev_free(ctx, d_rq);
  bgn_dev_free(ctx, d_ct);
  bgn_dev_free(ctx, d_nonce);
  bgn_dev_free(ctx, d_dl);
  bgn_dev_free(ctx, d_c);
  bgn_dev_free(ctx, d_ok);
  bgn_ctx_destroy(ctx);
  printf("cgo_shape_proofs: %zu proofs, %d failures\n", count, failures);
  return failures ? 1 : 0;
}
