"""The proof that tests/test_encoder_sharp_gpu.py can fail: on the CPU, in float64, every named defect of
oracle/encoder_probe.py moves the output of every case of tests/encoder_cases.py by a multiple of the tolerance the GPU
test grants.

Per case and layer boundary, ``floor`` = error of probe(rounding="bf16") against probe(exact) in two metrics over all
live tokens (``row_rel``: max over tokens of ||delta row|| / ||reference row||; ``max_abs``), and ``TOL`` = 2 x floor
(encoder_cases.tolerances; the factor 2 is a condition of the design, see there).  A must-catch defect has to reach
4 x TOL = 8 x floor in at least one metric at layer boundary 1, where every defect first becomes observable (an encoder
handle needs at least one layer, so embedding defects are seen through layer 1): a GPU result anywhere up to TOL is then
still told apart from the defect by a factor of 3.

Must-catch: all cases: uniform_softmax, no_scale, scale_half, pos_plus_one, leak_prev_sequence, drop_last_key, and the
wrong LayerNorm eps on the low-variance tokens (bf16 cases); BERT: no_token_type; MPNet: no_rel_bias, rel_bias_swapped, bucket_plus_one,
rel_bias_heads_reversed, mpnet_pos_ignores_pad; bf16 cases: no_q_bias, no_v_bias, no_o_bias.
Smallest must-catch ratio (error / TOL, better metric) per case as measured: tiny-bert 6.8 (drop_last_key), tiny-mpnet
15.9, bert-384 8.7, mpnet-384 15.9, bert-768 6.5, mpnet-768 10.8 (no_o_bias in these four), bert-768-mxfp8 4.4,
mpnet-768-mxfp8 7.0 (drop_last_key); wrong eps 15.7-24.5 (bf16 cases).

The cases of tests/config_cases.py (the accepted configurations no other case reaches) get the same must-catch list and two
defects more: ffn_tail_dropped in every one of them, drop_last_head_group where heads % 4 != 0.  Smallest must-catch ratio as
measured: bert-64-h2-f64 7.3 (ffn_tail_dropped), mpnet-64-h1-f320 5.4 (drop_last_key), bert-384-h6-f768 10.6,
bert-384-h24-f1920 12.6 (no_o_bias), bert-384-f1024 11.5 (no_v_bias), bert-384-f2112 10.4 (no_o_bias), mpnet-384-h6-f2048 13.3
(ffn_tail_dropped), bert-768-h24-f1920 8.0, bert-768-h48-f1984 7.3 (no_o_bias), bert-768-h24-f2048-mxfp8 4.8 (drop_last_key),
bert-1024-h32-f2816 4.7 (no_o_bias); ffn_tail_dropped 7.3-19.4 (MXFP8 case 5.1 with config_cases.F2_TAIL, 1.5 without),
drop_last_head_group 38.7-79.7; wrong eps 11.4-31.8 (bf16 cases; MXFP8 case 3.8, reported as for the other MXFP8 cases).
mpnet-64-h1-f320 has one head: rel_bias_heads_reversed is the identity there (asserted: the error is exactly 0), so that
case cannot carry it; mpnet-384-h6-f2048 carries it for the partial head group with a relative bias (ratio 50.8).

NOT claimed (ratio = error / TOL, better metric, as measured by this file; printed on every run):
* no_k_bias: the softmax is invariant to q.b_k, which is the same for every key of a query.  Asserted: in float64 the
  error is rounding noise (<= 1e-9; measured 1e-14), which documents why no test can see a dropped key bias.
* gelu_tanh for erf-GELU: ratio 0.00-0.04 in every case: below bf16 resolution.
* var_unbiased: hidden 64: ratio 1.0-1.1.  The variance changes by 1/64, a row by 0.8 %, against a rounding floor of
  0.5-0.8 % of a row; both scale with the row, so no choice of weights separates them, and the defect left the must-catch
  list.  Hidden 384 and 768: ratio 0.09-0.17 (MXFP8: 1.0-1.3).
* MXFP8 cases, projection biases: the floor is ~6x the bf16 one.  no_q_bias reaches ratio 8.8 / 12.8, no_v_bias 2.1 / 3.1,
  no_o_bias 1.1 / 1.3; reported, not asserted.  The projections' bias path is the bf16 cases' claim.
* MXFP8 cases, wrong LayerNorm eps: ratio 3.3 / 3.4 (bf16 cases 15.7-24.5).  The embedding LayerNorm kernel does not depend on
  the weight format, so the bf16 cases carry this claim.  With var_unbiased at hidden 64 this is the second and last
  defect that left the must-catch list.
"""
import numpy as np
import pytest

import config_cases as cc
import encoder_cases as ec

ALL_CASES = list(ec.CASES) + list(cc.CASES)


def case(name):
    return ec.CASES[name] if name in ec.CASES else cc.CASES[name]


def case_inputs(name):
    return ec.case_inputs(name) if name in ec.CASES else cc.inputs(name)


def case_weights(name):
    return ec.sharp_weights(ec.CASES[name][0], name) if name in ec.CASES else cc.weights(name)


def probe(name, **kw):
    return ec.probe(name, **kw) if name in ec.CASES else cc.probe(name, **kw)


def tolerances(name):
    return ec.tolerances(name) if name in ec.CASES else cc.tolerances(name)


ATTENTION = ["uniform_softmax", "no_scale", "scale_half", "leak_prev_sequence", "drop_last_key"]
REL_BIAS = ["no_rel_bias", "rel_bias_swapped", "bucket_plus_one", "rel_bias_heads_reversed"]
PROJ_BIAS = ["no_q_bias", "no_v_bias", "no_o_bias"]


def must_catch(name):
    cfg, wd = case(name)
    d = ATTENTION + ["pos_plus_one"]
    d += ["no_token_type"] if cfg.arch == "bert" else REL_BIAS + ["mpnet_pos_ignores_pad"]
    if wd == "bf16":
        d += PROJ_BIAS
    if name in cc.CASES:
        d += ["ffn_tail_dropped"] + (["drop_last_head_group"] if cfg.heads % 4 else [])
        if cfg.heads == 1:      # the identity there (asserted in test_every_defect_stands_above_the_tolerance)
            d.remove("rel_bias_heads_reversed")
    return d


def reported(name):
    cfg, wd = case(name)
    return ["gelu_tanh", "var_unbiased"] + (PROJ_BIAS if wd != "bf16" else [])


def ratio(got, exact, tol):
    e = ec.errors(got, exact)
    return max(e[m] / tol[m] for m in ec.METRICS), e


def wrong_eps(name):
    return "eps_1e-5" if case(name)[0].arch == "bert" else "eps_1e-12"


@pytest.mark.parametrize("name", ALL_CASES)
def test_weights_make_every_stage_matter(name):
    """The conditions ``sharp_weights`` promises, measured with the float64 probe on the case's own inputs."""
    from oracle import encoder_probe
    cfg, wd = case(name)
    ids, cu, notes = case_inputs(name)
    w = case_weights(name)
    assert all(np.array_equal(v, ec.presets.bf16_round(v)) for k, v in w.items() if "word_embeddings" not in k)
    st = {}
    encoder_probe.probe_forward(cfg, w, ids, cu, linear=ec.fp8_ref.mx_linear if wd == "mxfp8" else None, stats=st)
    live = int((np.diff(cu) > 0).sum())
    for l in range(cfg.num_layers):
        per_seq = st["softmax_max"][l * live:(l + 1) * live]
        med = float(np.median(np.concatenate([v for S, v in per_seq if S >= 16])))
        print(f"{name} layer {l + 1}: median largest probability {med:.3f}, max |FFN1 pre-activation| {st['ffn1_absmax'][l]:.1f}")
        assert 0.2 <= med <= 0.9
        assert st["ffn1_absmax"][l] >= 3.0
    # the LayerNorm-eps tokens: embedding-LayerNorm input variance below 1e-5 and above 1e-12
    s = notes["lowvar"]
    tok = ids[cu[s]:cu[s + 1]].astype(np.int64)
    pos, _ = encoder_probe.packed_positions(cfg, ids, cu)
    x = w["embeddings.word_embeddings.weight"][tok].astype(np.float64) + w["embeddings.position_embeddings.weight"][pos[cu[s]:cu[s + 1]]]
    if cfg.arch == "bert":
        x = x + w["embeddings.token_type_embeddings.weight"][0]
    assert (x.var(1) < 2e-6).all() and (x.var(1) > 5e-7).all()


@pytest.mark.parametrize("name", ALL_CASES)
def test_every_defect_stands_above_the_tolerance(name):
    cfg, wd = case(name)
    ids, cu, notes = case_inputs(name)
    exact, floor, tol = tolerances(name)
    for b in list(range(1, cfg.num_layers + 1)) + ["pooled"]:
        print(f"{name} boundary {b}: " + "  ".join(f"{m} floor {floor[b][m]:.4g} TOL {tol[b][m]:.4g}" for m in ec.METRICS))
        assert all(floor[b][m] > 0 for m in ec.METRICS)
    smallest = (np.inf, None)
    for d in must_catch(name):
        r, e = ratio(probe(name, defect=d, num_layers=1)[1], exact[1], tol[1])
        print(f"{name} {d:26s} row_rel {e['row_rel']:.4g} max_abs {e['max_abs']:.4g}  ratio to TOL {r:.1f}")
        smallest = min(smallest, (r, d))
        assert r >= ec.POWER_FACTOR, f"{name}: defect {d} reaches only {r:.2f} x TOL"
    print(f"{name}: smallest must-catch ratio {smallest[0]:.1f} ({smallest[1]})")
    for d in reported(name):
        r, e = ratio(probe(name, defect=d, num_layers=1)[1], exact[1], tol[1])
        print(f"{name} {d:26s} row_rel {e['row_rel']:.4g} max_abs {e['max_abs']:.4g}  ratio to TOL {r:.2f}  (reported, not claimed)")
    if wd == "bf16":   # a dropped key bias is invisible: q.b_k is one constant per query
        e = ec.errors(probe(name, defect="no_k_bias", num_layers=1)[1], exact[1])
        print(f"{name} no_k_bias: max_abs {e['max_abs']:.3g} (float64 noise)")
        assert e["max_abs"] <= 1e-9
    if cfg.arch == "mpnet" and cfg.heads == 1:   # one head reversed is the same head: not a defect of this case
        assert ec.errors(probe(name, defect="rel_bias_heads_reversed", num_layers=1)[1], exact[1])["max_abs"] == 0.0


@pytest.mark.parametrize("name", ALL_CASES)
def test_wrong_layernorm_eps_moves_the_low_variance_tokens(name):
    """Embedding-LayerNorm input variance 9.5e-7 sits between the two eps values, so the other architecture's eps scales
    those rows by 3.4 (or 1/3.4).  Seen after layer 1 on those tokens.  Asserted for the bf16 cases; reported for the MXFP8
    ones, whose floor is ~6x larger (the embedding kernel is the same for both weight formats)."""
    cfg, wd = case(name)
    ids, cu, notes = case_inputs(name)
    exact, floor, tol = tolerances(name)
    s = notes["lowvar"]
    rows = slice(int(cu[s]), int(cu[s + 1]))
    got = probe(name, defect=wrong_eps(name), num_layers=1)[1]
    r, e = ratio(got[rows], exact[1][rows], tol[1])
    print(f"{name} {wrong_eps(name)} on the low-variance tokens: row_rel {e['row_rel']:.4g} max_abs {e['max_abs']:.4g} "
          f"(TOL {tol[1]['row_rel']:.4g} / {tol[1]['max_abs']:.4g})  ratio {r:.1f}" + ("" if wd == "bf16" else "  (reported, not claimed)"))
    if wd == "bf16":
        assert r >= ec.POWER_FACTOR
