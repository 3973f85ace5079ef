"""Layout generator with the reference's constructor (models_clevr/nmn3_netgen_att.py:46-71):

    AttentionSeq2Seq(input_seq_batch[T,N] i32, seq_length_batch[N] i32, T_decoder, num_vocab_txt,
                     embed_dim_txt, num_vocab_nmn, embed_dim_nmn, lstm_dim, num_layers, assembler,
                     encoder_dropout, decoder_dropout, decoder_sampling, use_gt_layout=None,
                     gt_layout_batch=None, scope='encoder_decoder', reuse=None)

Attributes `.predicted_tokens .token_probs .neg_entropy .atts .word_vecs` (:305-322) are fetch
handles; `run(feeds)` executes phase 1 through the C-ABI (`n2nmn_seq2seq_forward`: 2-layer LSTM
encoder, attentional LSTM decoder under the validity automaton, text-attention word vectors) and
returns device tensors.  Inputs may be placeholders (bound by `feeds`) or tensors.  Extra keyword
`beam_size=` (default 1): decode the layout by beam search of that width (include/n2nmn.h section 2b).
"""
from __future__ import annotations

from .engine import Engine
from .runtime import Fetch, Phase1Inputs, SamplingUniforms
from .train import DropoutStream

PHASE1_OUTPUTS = ('predicted_tokens', 'token_probs', 'neg_entropy', 'atts', 'word_vecs',
                  'log_seq_prob')


class AttentionSeq2Seq:
    def __init__(self, input_seq_batch, seq_length_batch, T_decoder, num_vocab_txt, embed_dim_txt,
                 num_vocab_nmn, embed_dim_nmn, lstm_dim, num_layers, assembler, encoder_dropout,
                 decoder_dropout, decoder_sampling, use_gt_layout=None, gt_layout_batch=None,
                 scope='encoder_decoder', reuse=None, engine: Engine = None, sample_seed: int = 0,
                 dropout_seed: int = 0, beam_size: int = 1):
        if engine is None:
            raise ValueError('AttentionSeq2Seq needs engine=Engine(...)')
        d = engine.dims
        want = dict(num_vocab_txt=num_vocab_txt, embed_dim_txt=embed_dim_txt,
                    num_vocab_nmn=num_vocab_nmn, embed_dim_nmn=embed_dim_nmn, lstm_dim=lstm_dim,
                    num_layers=num_layers)
        for k, v in want.items():
            if getattr(d, k) != v:
                raise ValueError('%s=%r differs from the engine dims (%r)' % (k, v, getattr(d, k)))
        if T_decoder > d.T_decoder:
            raise ValueError('T_decoder exceeds the engine capacity')
        # encoder_dropout / decoder_dropout: DropoutWrapper(output_keep_prob=0.5) on the output of every
        # LSTM layer but the last (:17-44) -> multipliers on layer 0's output, handed to the C-ABI as
        # n2nmn_seq2seq_io.drop_enc0 / drop_dec0.  (Inactive in every CLEVR script of the reference,
        # train_clevr_gt_layout.py:31-32, but part of the constructor contract.)
        self.dropout_masks = None      # {'enc0': [T_enc, N, L], 'dec0': [T_dec, N, L]} {0,1} keep masks
        #                                for every run (tests: TF's RNG stream is not reproducible);
        #                                None: drawn from the counter-based stream (dropout_seed)
        self.dropout_stream = DropoutStream(engine, 0.5, dropout_seed)
        self.engine = engine
        self.T_decoder = T_decoder
        self.encoder_num_vocab = num_vocab_txt
        self.encoder_embed_dim = embed_dim_txt
        self.decoder_num_vocab = num_vocab_nmn
        self.decoder_embed_dim = embed_dim_nmn
        self.lstm_dim = lstm_dim
        self.num_layers = num_layers
        self.EOS_token = assembler.EOS_idx
        self.P, self.W, self.b = assembler.P, assembler.W, assembler.b
        self.encoder_dropout = encoder_dropout
        self.decoder_dropout = decoder_dropout
        self.decoder_sampling = decoder_sampling
        self.phase1_inputs = Phase1Inputs(input_seq_batch, seq_length_batch, use_gt_layout, gt_layout_batch)
        self.sampling = SamplingUniforms(sample_seed)
        # extra keyword behind the reference's arguments: layouts by beam search of this width on the device
        # (Engine.seq2seq beam_size; 1 = the reference's greedy / sampled decoding)
        self.beam_size = int(beam_size)
        for name in PHASE1_OUTPUTS:
            setattr(self, name, Fetch(self, name, 1))

    def run(self, feeds=None, forced_tokens=None, debug=False):
        """Execute phase 1; returns {name: device tensor}."""
        import torch
        seq, lens, use_gt, gt = self.phase1_inputs.resolve(feeds or {})
        T, n = torch.as_tensor(seq).shape
        uni = self.sampling.draw(self.T_decoder, n, self.engine.device) if self.decoder_sampling else None
        shapes = dict(enc0=(T, n, self.lstm_dim), dec0=(self.T_decoder, n, self.lstm_dim))
        on = dict(enc0=self.encoder_dropout, dec0=self.decoder_dropout)
        mult = self.dropout_stream.multipliers({k: s for k, s in shapes.items() if on[k]}, self.dropout_masks)
        return self.engine.seq2seq(seq, lens, self.T_decoder, use_gt, gt, uni, forced_tokens, debug=debug,
                                   dropout=(mult.get('enc0'), mult.get('dec0')), beam_size=self.beam_size)

    def _fetch(self, f, handle):
        from .runtime import to_numpy
        if handle.phase1 is None:
            handle.phase1 = self.run(handle.feeds)
        return to_numpy(handle.phase1[f.name])
