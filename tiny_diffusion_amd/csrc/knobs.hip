// tdx_tune_set / tdx_tune_get / tdx_tune_name: the key table over TdxKnobs (knobs.h).  Touches no device.
#include <climits>
#include <cstring>
#include "common.h"
#include "knobs.h"

TdxKnobs g_knobs;

namespace {
// how a key stores a value v:  RAW v | BOOL v != 0 | MASK v & a | AT_LEAST max(v, a) | RANGE v if a <= v <= b, else
// the default | BIT sets or clears the bits a of the field (and a get answers whether they are set)
enum Norm { RAW, BOOL, MASK, AT_LEAST, RANGE, BIT };
struct Knob { const char* name; int TdxKnobs::*field; Norm norm; int a, b; };
#define K(key, ...) {#key, &TdxKnobs::key, __VA_ARGS__}
#define POSITIVE RANGE, 1, INT_MAX
#define NON_NEGATIVE RANGE, 0, INT_MAX
const Knob kKnobs[] = {
    K(conv_tile, RAW), K(splitk, RAW), K(splitk_tiles, RAW), K(splitk_target, RAW), K(streams, RAW),
    K(materialize, RAW), K(sample_defer_max, RAW), K(conv_dbg, RAW), K(conv_stamp, RAW), K(wgrad_small, RAW),
    K(bf16_storage, BOOL), K(sample_tables, BOOL), K(sample_halves, BOOL), K(conv_hybrid, BOOL), K(splitk_train, BOOL),
    K(bf16_materialize, BOOL), K(bf16_ring, BOOL), K(bf16_wgrad9, BOOL), K(bf16_wgrad_swz, BOOL), K(wino, BOOL),
    K(wino_infer, BOOL), K(wino_wgrad, BOOL), K(wino_rows, BOOL), K(infer_ring, BOOL),
    K(sample_fuse, MASK, 7), K(bnbwd_fused, MASK, 7),
    K(conv_min_tiles, POSITIVE), K(splitk_train_t64, POSITIVE), K(splitk_train_target, POSITIVE),
    K(wino_wgrad_min_tiles, POSITIVE), K(wino_wgrad_target, POSITIVE), K(wino_rows_min_stages, POSITIVE),
    K(wgrad_target, POSITIVE),
    K(wino_infer_min_units, NON_NEGATIVE), K(wino_infer_ovh, NON_NEGATIVE), K(wino_infer_red, NON_NEGATIVE),
    K(infer_ovh, NON_NEGATIVE), K(infer_red, NON_NEGATIVE),
    K(infer_stages, RANGE, 3, 4), K(infer_cus, RANGE, 1, 256),
    K(wino_min_wgs, AT_LEAST, 1), K(wgrad_target_big, AT_LEAST, 0), K(infer_splits, AT_LEAST, 0),
    K(wgrad9_wgs, AT_LEAST, 0), K(sample_halves_min, AT_LEAST, 2), K(bf16_thin, AT_LEAST, 0),
    {"stats_epi", &TdxKnobs::conv_dbg, BIT, 8},
};
#undef K
#undef POSITIVE
#undef NON_NEGATIVE
const int kCount = sizeof kKnobs / sizeof *kKnobs;

const Knob* find(const char* key) {
  for (int i = 0; key && i < kCount; ++i)
    if (!strcmp(key, kKnobs[i].name)) return &kKnobs[i];
  return nullptr;
}
}  // namespace

extern "C" int tdx_tune_set(const char* key, int value) {
  const Knob* k = find(key);
  if (!k) return TDX_E_BADARG;
  int& f = g_knobs.*k->field;
  switch (k->norm) {
    case RAW: f = value; break;
    case BOOL: f = value != 0; break;
    case MASK: f = value & k->a; break;
    case AT_LEAST: f = value > k->a ? value : k->a; break;
    case RANGE: f = value >= k->a && value <= k->b ? value : TdxKnobs{}.*k->field; break;
    case BIT: f = value ? (f | k->a) : (f & ~k->a); break;
  }
  return 0;
}

extern "C" int tdx_tune_get(const char* key, int* value) {
  const Knob* k = find(key);
  if (!k || !value) return TDX_E_BADARG;
  const int f = g_knobs.*k->field;
  *value = k->norm == BIT ? (f & k->a) != 0 : f;
  return 0;
}

extern "C" const char* tdx_tune_name(int index) { return index >= 0 && index < kCount ? kKnobs[index].name : nullptr; }
