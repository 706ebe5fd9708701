"""Evaluation: the forward-only path, replayed, with the accuracy counted on the device.

The reference scores dev and test after every epoch (qagnn.py:30-38: model.eval(), torch.no_grad(), one `.item()` per batch).  Here

  * the k-hop stack of an eval forward keeps nothing a backward would read and runs its large products in the three-MFMA form
    (ops.inference_path -> ops.stack_infer -> qagnn_stack_infer_f32, include/qagnn_hip_infer.h);
  * `GraphedForward` replays the decoder's eval forward as ONE hipGraph launch -- at the reference's eval batch of a few questions the
    eager forward is bound by the host, exactly like the training step graphed.GraphedStep replays;
  * predictions are compared with the labels by a kernel (qagnn_choice_eval_f32) into two device counters that the host reads once,
    after the last batch.

Nothing here touches BatchNorm buffers, dropout seeds, the seed epoch or a `.grad`.
"""
import torch

from . import graphed, ops
from .graphed import edge_capacity


class _Captured:
    __slots__ = ('graph', 'sent', 'cids', 'nt', 'ns', 'al', 'labels', 'packed', 'logits', 'attn', 'replays', 'watched', 'tables')


class GraphedForward:
    """fwd = GraphedForward(model, num_choice);  logits = fwd(sent_vecs, concept_ids, node_type_ids, node_scores, adj_lengths, packed,
    labels=None) -- the flattened [B, ...] decoder inputs of QAGNN.forward and the graph as graphed.GraphedStep takes it (a
    data_utils.PackedGraphBatch, EdgeListBatch or StoreBatch, or the plain (edge_index, edge_type) int64 pair); labels [B / num_choice]
    int64 or None.  Returns the static logits [B, 1] of the capture (overwritten by the next call).

    The captured work is QAGNN.forward in eval mode under torch.no_grad() and ops.inference_path(), then qagnn_choice_eval_f32 into
    counters this object owns: counts() -> (correct, seen) is the only host synchronisation, reset_counts() zeroes them.  One capture per
    (B, n, sent_dim, edge-capacity bucket, kind of graph input, labels or not); static inputs, warm-up, capture, the one-stream fallback
    and the validation flags read one call late are graphed.GraphedStep's (the helper functions of qagnn_amd/graphed.py)."""

    def __init__(self, model, num_choice, capacity=edge_capacity, warmup=2):
        self.model, self.nc, self.capacity, self.warmup = model, int(num_choice), capacity, int(warmup)
        self.dev = next(model.parameters()).device
        assert self.dev.type == 'cuda', 'GraphedForward captures a HIP graph: the model must live on the GPU'
        self._captured = {}
        self._pool = None
        self._counts = torch.zeros(2, dtype=torch.long, device=self.dev)
        self.overlap = True  # graph preparation on its side stream inside the capture; switched off if a capture rejects it

    # -- the eager forward that gets captured --------------------------------------------------------------------------------------
    def _forward(self, c):
        graphed.fetch_own_fields(c)
        with torch.no_grad(), ops.inference_path():
            logits, attn = self.model(c.sent, c.cids, c.nt, c.ns, c.al, c.packed)
        ops.kernels().choice_eval(logits.view(-1, self.nc), c.labels, self._counts)
        return logits, attn

    def _key(self, sent, cids, packed, labels):
        B, n = graphed.capture_dims(cids, packed)
        return (B, n, sent.size(1), int(self.capacity(packed.E)), packed.capture_kind(), labels is not None)

    def _capture(self, key, args):
        B, n, sent_dim, e_cap = key[:4]
        packed, labels = args[5], args[6]
        dev = self.dev
        c = _Captured()
        c.watched, c.tables = [], []
        c.sent = torch.empty((B, sent_dim), dtype=torch.float32, device=dev)
        graphed.alloc_static_fields(c, packed, B, n, dev)
        c.labels = torch.empty((B // self.nc,), dtype=torch.long, device=dev) if labels is not None else None
        c.packed = packed.static_twin(B, n, e_cap, dev)
        c.replays = 0
        self._load(c, args)
        held = self._counts.clone()  # (the warm-up forwards count their batch: put back afterwards)
        old = ops.PREP_OVERLAP
        ops.PREP_OVERLAP = ops.PREP_OVERLAP and self.overlap
        try:
            graphed.warm_up(dev, self.warmup, lambda: self._forward(c))
            self._counts.copy_(held)
            if self._pool is None:
                self._pool = torch.cuda.graph_pool_handle()
            c.graph, (c.logits, c.attn) = graphed.capture_graph(self._pool, c.watched, lambda: self._forward(c), c.tables)
        finally:
            ops.PREP_OVERLAP = old
        self._captured[key] = c
        return c

    @staticmethod
    def _load(c, args):
        sent, cids, nt, ns, al, packed, labels = args
        if c.labels is not None:
            c.labels.copy_(labels, non_blocking=True)
        graphed.load_static_inputs(c, sent, cids, nt, ns, al, packed)

    def __call__(self, sent_vecs, concept_ids, node_type_ids, node_scores, adj_lengths, packed, labels=None):
        if self.model.training:
            raise RuntimeError('GraphedForward replays the EVAL forward: call model.eval() first (a train-mode forward draws dropout '
                               'masks and updates BatchNorm buffers; graphed.GraphedStep replays that one)')
        packed = graphed.as_holder(packed, 'GraphedForward')
        args = (sent_vecs, concept_ids, node_type_ids, node_scores, adj_lengths, packed, labels)
        key = self._key(sent_vecs, concept_ids, packed, labels)
        with torch.cuda.device(self.dev):
            c = self._captured.get(key)
            if c is None:
                c = graphed.capture_or_fall_back(self, 'GraphedForward', lambda: self._capture(key, args))
            graphed.replay(c, lambda: self._load(c, args))
        return c.logits

    def reset_counts(self):
        self._counts.zero_()

    def counts(self):
        """(correct, seen) over the calls since reset_counts(): the one device-to-host copy of an evaluation"""
        correct, seen = self._counts.tolist()
        return correct, seen

    @property
    def n_graphs(self):
        return len(self._captured)


def evaluate_accuracy(eval_set, model, graphed=False):
    """The reference's evaluate_accuracy (qagnn.py:30-38): `for qids, labels, *input_data in eval_set`, model.eval(), no autograd,
    returns n_correct / n_samples (ZeroDivisionError on an empty set, as there) -- with the forward on the inference path and the two
    counts accumulated on the device: one synchronisation at the end instead of one per batch.  Leaves the model in eval mode, as the
    reference does.

    model: an LM_QAGNN (logits [bs, nc]; the encoder runs eagerly) or a QAGNN decoder (flattened inputs, logits [B, 1]: the number of
    choices is B / len(labels)).  graphed: for a decoder-level set, one hipGraph launch per batch -- True builds a GraphedForward for
    this pass; a GraphedForward of `model` (kept by the caller across the epochs' passes: its captures are made once) is used as it
    is, its counters zeroed first."""
    model.eval()
    fwd = graphed if isinstance(graphed, GraphedForward) else None
    assert fwd is None or fwd.model is model, 'the GraphedForward handed in replays another model'
    if fwd is not None:
        fwd.reset_counts()
    counts = None
    with torch.no_grad(), ops.inference_path():
        for qids, labels, *input_data in eval_set:
            if graphed:
                if fwd is None:
                    fwd = GraphedForward(model, input_data[0].size(0) // labels.size(0))
                fwd(*input_data, labels=labels)
                continue
            logits, _ = model(*input_data)
            if counts is None:
                counts = torch.zeros(2, dtype=torch.long, device=logits.device)
            ops.kernels().choice_eval(logits.reshape(labels.size(0), -1), labels.to(logits.device, non_blocking=True).contiguous(), counts)
    n_correct, n_samples = fwd.counts() if graphed and fwd is not None else (counts.tolist() if counts is not None else (0, 0))
    return n_correct / n_samples


def evaluate_detail(eval_set, model, preds_path=None, trace=False, head=-1):
    """The reference's detailed evaluation (qagnn.py:401-430, and the save_test_preds branch of its training loop, :294-310): the loop
    `for qids, labels, *input_data in eval_set` on the inference path, one prediction per question.  -> (accuracy, [(qid, pred)], traces):
    pred the index of the chosen answer, traces None or, with trace=True, one explain.Trace per batch (the attention of the forward's k
    hops followed out of the context node; head as explain.trace takes it).  preds_path: the reference's prediction file is written
    there, one line '{qid},{letter}' per question.

    The predictions are the argmax of qagnn_choice_eval_f32, kept on the device per batch; the two counts are accumulated there as in
    evaluate_accuracy; the host reads everything with ONE synchronisation behind the last batch (the reference: two `.item()` per
    question).  An empty set raises ZeroDivisionError, as evaluate_accuracy does.  Leaves the model in eval mode."""
    from . import explain
    model.eval()
    counts, preds, words, qid_list, traces = None, [], [], [], ([] if trace else None)
    K = ops.kernels()
    with torch.no_grad(), ops.inference_path():
        for qids, labels, *input_data in eval_set:
            if trace:
                rec, w = explain.trace_nosync(model, input_data, head)
                logits = rec.logits
                traces.append(rec)
                words.append(w[:1].to(logits.device))
            else:
                logits, _ = model(*input_data)
            if counts is None:
                counts = torch.zeros(2, dtype=torch.long, device=logits.device)
            Q = labels.size(0)
            pred = torch.empty(Q, dtype=torch.long, device=logits.device)
            K.choice_eval(logits.reshape(Q, -1), labels.to(logits.device, non_blocking=True).contiguous(), counts, pred=pred)
            preds.append(pred)
            qid_list += list(qids)
    host = torch.cat([counts] + preds + words).tolist() if counts is not None else [0, 0]  # the one device-to-host copy of the pass
    n_correct, n_samples = host[:2]
    accuracy = n_correct / n_samples
    for flag in host[2 + len(qid_list):]:
        explain.check_block_flag(flag)
    results = list(zip(qid_list, host[2:2 + len(qid_list)]))
    if preds_path is not None:
        with open(preds_path, 'w') as f:
            for qid, p in results:
                print('{},{}'.format(qid, chr(ord('A') + p)), file=f)  # (qagnn.py:307)
    return accuracy, results, traces
