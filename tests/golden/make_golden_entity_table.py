#!/usr/bin/env python
"""Golden vectors for a TRAINABLE entity table, from the REFERENCE's own QAGNN built with freeze_ent_emb=False (modeling_qagnn.py:103-110,
utils/layers.py:573-584), run in the authoring container.  Writes tests/golden/entity_table.npz: for the shapes of `small_train`
(table 300 x 16) and `config1_train` (1000 x 32), on the inputs of those fixtures and the same seeded weights, the logits and the full
gradient of the table under loss = sum(logits * linspace(0.5, 1.5)) -- what nn.Embedding hands the optimiser."""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

CASES = ('small_train', 'config1_train')


def main():
    import helpers
    from make_golden import import_reference
    _, ref_mq = import_reference()
    torch.set_num_threads(8)
    out = {}
    for name in CASES:
        c = helpers.GOLDEN_CASES[name]
        cfg = c['cfg']
        B = c['nq'] * c['nc']
        sv, cids, nt, ns, al, ei, et = helpers.golden_inputs(name, helpers.load_golden(name))
        torch.manual_seed(0)
        model = ref_mq.QAGNN(None, cfg['k'], cfg['n_ntype'], cfg['n_etype'], cfg['sent_dim'], cfg['n_concept'], cfg['concept_dim'],
                             cfg['concept_in_dim'], cfg['n_attention_head'], cfg['fc_dim'], cfg['n_fc_layer'], cfg['p_emb'], cfg['p_gnn'],
                             cfg['p_fc'], pretrained_concept_emb=None, freeze_ent_emb=False, init_range=cfg['init_range'])
        helpers.det_fill_(model, c['seed'], c['std'])
        model.pooler.dropout.p = 0.0
        model.pooler.attention.dropout.p = 0.0
        model.train(c['train'])
        assert model.concept_emb.emb.weight.requires_grad
        logits, _ = model(sv, cids, nt, ns, al, (ei, et))
        (logits * torch.linspace(0.5, 1.5, B).view(B, 1)).sum().backward()
        out[name + '::logits'] = logits.detach().numpy()
        out[name + '::grad::concept_emb.emb.weight'] = model.concept_emb.emb.weight.grad.numpy()
        out[name + '::grad::concept_emb.cpt_transform.weight'] = model.concept_emb.cpt_transform.weight.grad.numpy()
    path = os.path.join(HERE, 'entity_table.npz')
    np.savez_compressed(path, **out)
    print('wrote entity_table.npz', {k: v.shape for k, v in out.items()}, f'{os.path.getsize(path) / 1024:.0f} KiB')


if __name__ == '__main__':
    main()
