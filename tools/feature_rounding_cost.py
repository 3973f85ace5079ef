#!/usr/bin/env python3
"""What `feature_dtype='float16'` costs in the logits: the full-size reference-code fixture of
tests/test_gpu_reference_fixture.py (N = 64, seed-0 weights, tests/golden/float_cases.py case 'full') run with its
features as given and with the same features rounded through IEEE half.  Prints the maximum logit difference, the
logits' scale and the number of questions whose arg-max changes, for ground-truth and for decoded layouts.
Recorded in profiles/feature_feed.md; the option stays opt-in whatever the figures are."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests', 'golden'))


def main():
    import float_cases as FC
    from n2nmn_amd import synth
    from n2nmn_amd.engine import Engine
    from n2nmn_amd.nmn3_assembler import Assembler
    from n2nmn_amd.spec import CLEVR_MODULE_NAMES
    d, batch = FC.clevr_inputs('full')
    eng = Engine(d, Assembler(list(CLEVR_MODULE_NAMES)))
    eng.load_weights(FC.clevr_weights())
    gt = synth.template_layout_batch(d)
    feat = batch['image_feat_batch']
    half = feat.astype(np.float16)
    rel = np.abs(half.astype(np.float32) - feat)[feat != 0] / np.abs(feat[feat != 0])
    print('features: N = %d, max |x| = %.3f, max relative rounding error %.3e (2^-11 = %.3e)'
          % (d.N, np.abs(feat).max(), rel.max(), 2.0 ** -11))
    for label, kw in (('ground-truth layouts', dict(use_gt_layout=True, gt_layout=gt)), ('decoded layouts', dict())):
        a, ta, _ = eng.forward(batch, **kw)
        a = a.cpu().numpy().copy()
        b, tb, _ = eng.forward(dict(batch, image_feat_batch=half), **kw)
        b = b.cpu().numpy().copy()
        assert np.array_equal(ta, tb)                  # (the layout does not depend on the image)
        diff = np.abs(a - b)
        print('%-22s max |logit diff| = %.3e (max |logit| = %.3f, mean |logit diff| = %.3e), arg-max changes: %d of %d'
              % (label + ':', diff.max(), np.abs(a).max(), diff.mean(), int((a.argmax(1) != b.argmax(1)).sum()), d.N))


if __name__ == '__main__':
    main()
