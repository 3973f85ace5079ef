"""fp64 beam search over the oracle's decoder, written for the tests from the oracle's own pieces
(oracle/n2nmn_oracle.py: encoder_forward, _lstm_cell, _lstm_w, _softmax, valid_tokens), with the semantics of
include/n2nmn.h section 2b:

* score of a prefix = sum of log(token_probs), token_probs = soft-max over all tokens, masked, renormalised
  (decoder_forward's own expressions, so a beam's score IS sum_t log token_probs of a forced-token run);
* step 0: beam 0 live (score 0), beams 1 .. K-1 score -inf;
* candidates (beam b, token s): score[b] + log p_b(s) if s is valid in b's automaton state and score[b] is
  finite, else -inf;
* total order: score descending, then beam ascending, then token ascending (-inf candidates included);
* the first K candidates are the beams of the next step, each with its parent's LSTM state;
* latch_eos (models_shapes): behind its first <eos> a beam's only candidate is <eos>, probability 1.

Rows are beam-major (row = b * N + n) like the engine's, but nothing depends on that here.
"""
import numpy as np

from oracle.n2nmn_oracle import _DEC, _cast, _lstm_cell, _lstm_w, _softmax, valid_tokens


def beam_search(w, enc, P, Wv, bv, T_dec, K, latch_eos=None, dtype=np.float64):
    """-> dict: tokens [K, T_dec, N] (final order, beam 0 = best), scores [K, N], parents [T_dec, K, N],
    step_tokens [T_dec, K, N], and the score gaps between candidates whose order decides something:
      gap_set [N]    smallest gap, over all steps, between the K-th candidate and the first one dropped (which
                     prefixes survive; the order INSIDE the kept K of an intermediate step only names the beams --
                     without exact ties the candidates of later steps and their scores do not depend on it)
      gap_final [N]  smallest gap between adjacent ranks inside the K beams after the last step (the final order)
      min_gap [N]    min of the two: a question is decidable at margin m iff min_gap >= m.
      gap_order [N]  smallest gap between ANY two adjacent ranks 0 .. K at ANY step: what must hold for the names
                     of the beams too (parents [T_dec, K, N], step_tokens) to be comparable.
    Pairs of two -inf candidates decide nothing (index order) and do not count."""
    w = _cast(w, dtype)
    (c0, h0), (c1, h1) = enc['states']
    N, L = h0.shape
    demb = w[_DEC + 'embedding_mat']
    V = demb.shape[0]
    v = w[_DEC + 'att_prediction/v']
    Wa, ba = w[_DEC + 'att_prediction/weights'], w[_DEC + 'att_prediction/biases']
    Wy, by = w[_DEC + 'token_prediction/weights'], w[_DEC + 'token_prediction/biases']
    W0, b0 = _lstm_w(w, 'decoder', 0)
    W1, b1 = _lstm_w(w, 'decoder', 1)
    eht, eout, nf = enc['h_transformed'], enc['outputs'], enc['not_finished']
    tile = lambda a: np.tile(np.asarray(a, dtype), (K, 1))
    c0, h0, c1, h1 = tile(c0), tile(h0), tile(c1), tile(h1)
    x = np.tile(w[_DEC + 'go_embedding'], (K * N, 1))
    X = np.tile(np.array([[0, 0, T_dec]], np.int64), (K * N, 1))
    seen = np.zeros(K * N, bool)
    score = np.full((K, N), -np.inf, dtype)
    score[0] = 0.0
    parents = np.zeros((T_dec, K, N), np.int32)
    step_tok = np.zeros((T_dec, K, N), np.int32)
    gap_set = np.full(N, np.inf)
    gap_final = np.full(N, np.inf)
    gap_order = np.full(N, np.inf)
    cols = np.arange(N)
    for t in range(T_dec):
        c0, h0 = _lstm_cell(x, c0, h0, W0, b0)
        c1, h1 = _lstm_cell(h0, c1, h1, W1, b1)
        out = h1
        q = out @ Wa + ba
        ctx = np.zeros_like(out)
        for b in range(K):                               # a beam's rows attend to their own question
            r = slice(b * N, (b + 1) * N)
            e = np.sum(np.tanh(q[r][None] + eht) * v, axis=2, keepdims=True)
            att = _softmax(e, axis=0) * nf
            att = att / np.sum(att, axis=0, keepdims=True)
            ctx[r] = np.sum(att * eout, axis=0)
        sc = np.concatenate([out, ctx], axis=1) @ Wy + by
        valid = valid_tokens(X, Wv, bv)
        vm = valid.astype(dtype)
        with np.errstate(divide='ignore', invalid='ignore'):
            p = _softmax(sc, axis=1) * vm
            p = p / np.sum(p, axis=1, keepdims=True)
            if latch_eos is not None:
                valid = np.where(seen[:, None], np.arange(V)[None, :] == latch_eos, valid)
                p = np.where(seen[:, None], (np.arange(V)[None, :] == latch_eos).astype(dtype), p)
            logp = np.where(valid, np.log(p), -np.inf)
        cand = score.reshape(K * N, 1) + logp            # [K N, V]
        cand = np.where(np.isnan(cand) | ~valid | np.isinf(score.reshape(K * N, 1)), -np.inf, cand)
        cand = cand.reshape(K, N, V).transpose(1, 0, 2).reshape(N, K * V)      # index = b * V + s
        order = np.argsort(-cand, axis=1, kind='stable')                        # ties: b, then s ascending
        srt = np.take_along_axis(cand, order, axis=1)
        hi, lo = srt[:, :K], srt[:, 1:K + 1]
        with np.errstate(invalid='ignore'):
            gap = np.where(np.isinf(hi) & np.isinf(lo), np.inf, hi - lo)
        gap_set = np.minimum(gap_set, gap[:, K - 1])
        gap_order = np.minimum(gap_order, gap.min(axis=1))
        if t == T_dec - 1:
            gap_final = gap[:, :K - 1].min(axis=1) if K > 1 else np.full(N, np.inf)
        pb, ps = order[:, :K] // V, order[:, :K] % V                           # [N, K]
        parents[t], step_tok[t] = pb.T, ps.T
        score = srt[:, :K].T.copy()
        src = (pb.T * N + cols[None, :]).reshape(K * N)                         # parent row of every new row
        tok = ps.T.reshape(K * N)
        c0, h0, c1, h1 = c0[src], h0[src], c1[src], h1[src]
        X = X[src] + P[tok]
        seen = seen[src] | (tok == latch_eos) if latch_eos is not None else seen
        x = demb[tok]
    tokens = np.zeros((K, T_dec, N), np.int32)
    cur = np.tile(np.arange(K)[:, None], (1, N))
    for t in range(T_dec - 1, -1, -1):
        tokens[:, t, :] = step_tok[t][cur, cols[None, :]]
        cur = parents[t][cur, cols[None, :]]
    return dict(tokens=tokens, scores=score, parents=parents, step_tokens=step_tok, gap_set=gap_set,
                gap_final=gap_final, min_gap=np.minimum(gap_set, gap_final), gap_order=gap_order)


def seq_log_prob(token_probs):
    """sum_t log token_probs [T, N], accumulated step by step like the search does"""
    s = np.zeros(token_probs.shape[1], token_probs.dtype)
    for t in range(token_probs.shape[0]):
        s = s + np.log(token_probs[t])
    return s


def all_layouts(P, Wv, bv, T_dec):
    """every token sequence of length T_dec the automaton accepts from (0, 0, T_dec) -> ([M, T_dec] int32,
    the largest number of valid prefixes at any step)"""
    prefixes = [((), np.array([0, 0, T_dec], np.int64))]
    widest = 1
    for _ in range(T_dec):
        nxt = []
        for toks, X in prefixes:
            for s in np.nonzero(valid_tokens(X[None], Wv, bv)[0])[0]:
                nxt.append((toks + (int(s),), X + P[s]))
        prefixes = nxt
        widest = max(widest, len(prefixes))
    return np.array([p[0] for p in prefixes], np.int32).reshape(len(prefixes), T_dec), widest
