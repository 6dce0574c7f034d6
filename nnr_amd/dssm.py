"""The DSSM baseline of the reference's general_recommendation_methods/ (DSSM_model.py, DSSM_main.py, DSSM_util.py, DSSM_dataset.py) on the
weighted-bag and cosine-loss kernels of csrc/dssm.hip.

The reference's forward gathers word_embedding rows for every tf-idf term of every user ([B, 3200, 512]) and every candidate ([B, N, 200,
512]), scales, drops and sums them: 550 MB of buffers at the default sizes for a [B + B N, 512] result.  Here both bags are ONE launch that
reads each live table row once and writes the stacked [B + B N, H] result; the two tanh layers run over the stacked rows (one GEMM each,
functional.LinearFn); the cosine head, the loss and their gradients are one launch; the table gradient is a sorted, atomic-free reduction.

Dropout sites, in the reference's order: the two bags (inside the kernel: seed + 1 for the user stream, seed + 2 for the news stream, index
((row * L + position) * H + column)), l3 over the stacked rows (seed + 3, flat over [B + B N, H]), y (seed + 4, flat over [B + B N, F]);
`seed` advances per call as the encoders' _next_seed does.  No CPU path: CPU tensors raise NnrHipError."""
import argparse

import numpy as np
import torch
import torch.nn as nn

from . import _lib as L
from . import functional as Fn
from . import ops
from .corpus import NegativeSampler, impression_lists, negative_sampling
from .evaluate import eval_mode
from .trainer import FlatParams


def make_dssm_config(argv=None):
    """The flags and defaults of DSSM_util.py:34-57 as a plain namespace; nothing else happens (no directories, no seeding, no device)."""
    p = argparse.ArgumentParser(description='DSSM')
    p.add_argument('--mode', type=str, default='train', choices=['train', 'dev', 'test', 'debug'])
    p.add_argument('--dev_model_path', type=str, default='best_model/DSSM/#1/DSSM')
    p.add_argument('--test_model_path', type=str, default='best_model/DSSM/#1/DSSM')
    p.add_argument('--device_id', type=int, default=0)
    p.add_argument('--seed', type=int, default=0)
    p.add_argument('--dataset', type=str, default='200k', choices=['200k', 'small', 'large'])
    p.add_argument('--news_word_num', type=int, default=200)
    p.add_argument('--user_word_num', type=int, default=3200)
    p.add_argument('--negative_sample_num', type=int, default=4)
    p.add_argument('--epoch', type=int, default=100)
    p.add_argument('--batch_size', type=int, default=64)
    p.add_argument('--lr', type=float, default=1e-4)
    p.add_argument('--weight_decay', type=float, default=0)
    p.add_argument('--gradient_clip_norm', type=float, default=4)
    p.add_argument('--dev_criterion', type=str, default='auc', choices=['auc', 'mrr', 'ndcg', 'ndcg10'])
    p.add_argument('--early_stopping_epoch', type=int, default=5)
    p.add_argument('--word_embedding_dim', type=int, default=300, choices=[50, 100, 200, 300])
    p.add_argument('--DSSM_hidden_dim', type=int, default=512)
    p.add_argument('--DSSM_feature_dim', type=int, default=512)
    p.add_argument('--dropout_rate', type=float, default=0)
    return p.parse_args([] if argv is None else list(argv))


class DssmCorpus:
    """Device-resident term-vector tables (DSSM_util.py:12-27: per user / news the `length` heaviest tf-idf terms, ids and weights, zero
    padded) plus the behaviours, so that a batch is ids only: (user_sel int32 [B], news_sel int32 [B, 1 + K]).
    user_ids / user_w [U, Lu], news_ids / news_w [M, Ln]: numpy or torch; behaviors (training): [(user row, clicked news row, [non-clicked
    news rows]), ...] one per positive; samples (dev / test): (user rows [n], news rows [n]), one per (impression, candidate)."""

    def __init__(self, user_ids, user_w, news_ids, news_w, device, behaviors=None, samples=None):
        dev = torch.device(device)
        self.device = dev
        ui, ni = np.asarray(user_ids), np.asarray(news_ids)
        self.vocabulary_size = int(max(ui.max(initial=0), ni.max(initial=0))) + 1          # DSSM_util.py:146-151
        self.user_ids = torch.as_tensor(ui.astype(np.int32)).contiguous().to(dev)
        self.news_ids = torch.as_tensor(ni.astype(np.int32)).contiguous().to(dev)
        self.user_w = torch.as_tensor(np.asarray(user_w, dtype=np.float32)).contiguous().to(dev)
        self.news_w = torch.as_tensor(np.asarray(news_w, dtype=np.float32)).contiguous().to(dev)
        assert self.user_ids.shape == self.user_w.shape and self.news_ids.shape == self.news_w.shape
        self.behaviors = list(behaviors) if behaviors is not None else []
        self.negatives = None
        self._sampler = None
        if samples is not None:
            self.sample_user = torch.as_tensor(np.asarray(samples[0], dtype=np.int32)).to(dev)
            self.sample_news = torch.as_tensor(np.asarray(samples[1], dtype=np.int32)).to(dev)
            self.num = int(self.sample_user.numel())

    def negative_sampling(self, negative_sample_num, randint=None):
        """Draw this epoch's negatives (corpus.negative_sampling, the rule of DSSM_dataset.py:53-66); host side, uploaded once."""
        randint = randint if randint is not None else np.random.randint
        table = negative_sampling([(c, n) for _, c, n in self.behaviors], negative_sample_num, randint)
        self.negatives = torch.as_tensor(table).to(self.device)
        self.beh_user = torch.as_tensor(np.asarray([u for u, _, _ in self.behaviors], dtype=np.int32)).to(self.device)
        return self.negatives

    def negative_sampling_device(self, negative_sample_num, epoch, seed=0):
        """Draw this epoch's negatives on the device (corpus.NegativeSampler: a pure function of (seed, epoch, behaviour), the rule of
        DSSM_dataset.py:53-66); the lists are uploaded on first use and `self.negatives` is rewritten in place afterwards."""
        if self._sampler is None:
            self._sampler = NegativeSampler(*impression_lists([(c, n) for _, c, n in self.behaviors]), self.device)
            self.beh_user = torch.as_tensor(np.asarray([u for u, _, _ in self.behaviors], dtype=np.int32)).to(self.device)
        self.negatives = self._sampler.draw(epoch, seed, negative_sample_num)
        return self.negatives

    def train_batch(self, beh_idx):
        """beh_idx: int tensor [B] of behaviour indices (device) -> (user_sel int32 [B], news_sel int32 [B, 1 + K])."""
        assert self.negatives is not None, 'call negative_sampling first'
        idx = beh_idx.long()
        return self.beh_user[idx].contiguous(), self.negatives[idx].contiguous()

    def gather(self, user_sel, news_sel):
        """The six tensors of the reference's DataLoader for an id-only batch (tests, and the comparison runs of tools/dssm_bench.py)."""
        B = user_sel.numel()
        ns = news_sel.reshape(B, -1).long()
        ui, uw = self.user_ids[user_sel.long()].long(), self.user_w[user_sel.long()]
        ni, nw = self.news_ids[ns].long(), self.news_w[ns]
        return ui, uw, (uw != 0).sum(dim=1).float(), ni, nw, (nw != 0).sum(dim=2).float()


class DSSM(nn.Module):
    def __init__(self, config):
        super().__init__()
        V, H, Fd = int(config.vocabulary_size), int(config.DSSM_hidden_dim), int(config.DSSM_feature_dim)
        Lu, Ln = int(getattr(config, 'user_word_num', 3200)), int(getattr(config, 'news_word_num', 200))
        # nnr_wbag_dims' rule (ops.wbag_supported restates it: no library call, no device); Ln >= 1: a news stream always exists
        if not ops.wbag_supported(H, Lu, Ln) or Ln < 1 or not 1 <= Fd:
            raise Exception('DSSM_hidden_dim=%d, user_word_num=%d, news_word_num=%d: %s' % (H, Lu, Ln, ops.WBAG_UNSUPPORTED))
        self.word_embedding = nn.Embedding(num_embeddings=V, embedding_dim=H)
        self.W3 = nn.Linear(in_features=H, out_features=H, bias=True)
        self.W4 = nn.Linear(in_features=H, out_features=Fd, bias=True)
        self.dropout_rate = float(config.dropout_rate)
        self.hidden_dim, self.feature_dim, self.user_word_num, self.news_word_num = H, Fd, Lu, Ln
        self._seed_base = int(getattr(config, 'seed', 0)) * 4973 + 61
        self._calls = 0

    def initialize(self):
        nn.init.uniform_(self.word_embedding.weight, -0.1, 0.1)
        nn.init.xavier_uniform_(self.W3.weight, gain=nn.init.calculate_gain('tanh'))
        nn.init.xavier_uniform_(self.W4.weight, gain=nn.init.calculate_gain('tanh'))

    def _next_seed(self):
        self._calls += 1
        return (self._seed_base + 7919 * self._calls) & 0x7FFFFFFF

    # ------------------------------------------------------------------------------------------------ towers
    def towers(self, sa, sb):
        """y [na + nb, F]: both towers over the stacked rows of the user stream `sa` and the news stream `sb` (ops._wstream triples)."""
        table = self.word_embedding.weight
        if not table.is_cuda:
            raise L.NnrHipError('nnr_amd.dssm needs device tensors (no CPU fallback on the product path)')
        p = self.dropout_rate if self.training else 0.0
        seed = self._next_seed()
        need_grad = torch.is_grad_enabled() and table.requires_grad
        x = Fn.WbagFn.apply(table, sa, sb, p, seed + 1, seed + 2, need_grad)
        l3 = Fn.LinearFn.apply(x, self.W3.weight, self.W3.bias, ops.ACT_TANH, p, seed + 3)
        return Fn.LinearFn.apply(l3, self.W4.weight, self.W4.bias, ops.ACT_TANH, p, seed + 4)

    @staticmethod
    def _tensor_streams(user_indices, user_weights, news_indices, news_weights):
        for t in (user_indices, user_weights, news_indices, news_weights):
            if not t.is_cuda:
                raise L.NnrHipError('nnr_amd.dssm needs device tensors (no CPU fallback on the product path)')
        B, N = news_indices.shape[0], news_indices.shape[1]
        sa = (ops.ids32(user_indices, B, -1), user_weights.float().reshape(B, -1).contiguous(), None)
        sb = (ops.ids32(news_indices, B * N, -1), news_weights.float().reshape(B * N, -1).contiguous(), None)
        return sa, sb, B, N

    @staticmethod
    def _id_streams(corpus, user_sel, news_sel):
        B = user_sel.numel()
        N = news_sel.numel() // B
        sa = (corpus.user_ids, corpus.user_w, ops.ids32(user_sel, B))
        sb = (corpus.news_ids, corpus.news_w, ops.ids32(news_sel, B * N))
        return sa, sb, B, N

    def _logits(self, sa, sb, B, N):
        y = self.towers(sa, sb).detach()
        logits = torch.empty((B, N), device=y.device, dtype=torch.float32)
        ops.cosine_loss(y[:B], y[B:], B, N, y.shape[1], logits)
        return logits

    def forward(self, user_indices, user_weights, user_seq_len, news_indices, news_weights, news_seq_len):
        """logits [B, N] (DSSM_model.py:28-37); the two seq_len arguments are accepted and ignored, as in the reference.  The logits carry
        no autograd graph: train through loss() / loss_ids() (DssmTrainer does)."""
        with torch.no_grad():
            return self._logits(*self._tensor_streams(user_indices, user_weights, news_indices, news_weights))

    def forward_ids(self, corpus, user_sel, news_sel):
        """forward for an id-only batch: rows `user_sel` [B] / `news_sel` [B, N] of `corpus`' term-vector tables (read in place)."""
        with torch.no_grad():
            return self._logits(*self._id_streams(corpus, user_sel, news_sel))

    def loss(self, user_indices, user_weights, user_seq_len, news_indices, news_weights, news_seq_len):
        """(logits [B, N], loss): loss = mean_b(-log_softmax(logits)[b, 0]) (DSSM_main.py:63), differentiable."""
        sa, sb, B, N = self._tensor_streams(user_indices, user_weights, news_indices, news_weights)
        return Fn.CosineLossFn.apply(self.towers(sa, sb), B, N)

    def loss_ids(self, corpus, user_sel, news_sel):
        sa, sb, B, N = self._id_streams(corpus, user_sel, news_sel)
        return Fn.CosineLossFn.apply(self.towers(sa, sb), B, N)


class DssmTrainer:
    """DSSM_main.py:55-69 for one batch: forward, loss, zero_grad, backward, clip_grad_norm_(gradient_clip_norm), Adam -- the autograd path
    over flat parameter / gradient buffers with the fused clip + Adam kernel (trainer.Trainer.optimizer_step's).  No launch tape, no data
    parallelism."""

    def __init__(self, model, config):
        self.model, self.config = model, config
        self.flat = FlatParams(model)
        self.m = torch.zeros_like(self.flat.flat)
        self.v = torch.zeros_like(self.flat.flat)
        self.sumsq = torch.zeros(1, device=self.flat.flat.device, dtype=torch.float32)
        self.step_count = 0
        self.gradient_clip_norm = float(config.gradient_clip_norm)
        self.lr, self.weight_decay = float(config.lr), float(config.weight_decay)

    def forward_backward(self, batch):
        """batch: the six tensors of DSSM.forward, or (corpus, user_sel, news_sel).  Leaves the gradients in the flat buffer."""
        model = self.model
        self.flat.zero_grad()
        if len(batch) == 3:
            sa, sb, B, N = model._id_streams(*batch)
        else:
            sa, sb, B, N = model._tensor_streams(batch[0], batch[1], batch[3], batch[4])
        y = model.towers(sa, sb)
        dev, F = y.device, y.shape[1]
        logits = torch.empty((B, N), device=dev, dtype=torch.float32)
        loss = torch.empty((), device=dev, dtype=torch.float32)
        dy = torch.empty_like(y)
        ws = torch.empty(B, device=dev, dtype=torch.float32)
        yd = y.detach()
        ops.cosine_loss(yd[:B], yd[B:], B, N, F, logits, loss, None, dy[:B], dy[B:], ws)
        y.backward(dy)
        ops.join_extra_streams()
        return logits, loss

    def grad_total_norm(self):
        return float(self.flat.grad.double().norm())

    def optimizer_step(self):
        self.step_count += 1
        ops.sumsq(self.flat.grad, self.sumsq)
        ops.clip_adam(self.flat.flat, self.flat.grad, self.m, self.v, self.sumsq, 1.0, self.gradient_clip_norm, self.lr, 0.9, 0.999, 1e-8,
                      self.weight_decay, self.step_count)
        ops.PARAM_EPOCH[0] += 1       # parameters changed behind torch's back: invalidate the derived weights

    def train_step(self, batch):
        """One optimizer step; returns (logits, loss) as device tensors, no host synchronisation."""
        logits, loss = self.forward_backward(batch)
        self.optimizer_step()
        return logits, loss


def compute_scores(model, corpus, batch_size, cache='auto'):
    """One score per (impression, candidate) sample of `corpus`, in dataset order (DSSM_util.py:193-209, N = 1): float32 [n] on the device.
    cache 'auto' / True: every distinct user and every distinct news of the split goes through its tower ONCE (in eval mode both towers
    are functions of the row alone), then each sample is the cosine of two gathered rows; False: the reference's per-sample form."""
    dev, n = corpus.device, corpus.num
    scores = torch.empty(n, device=dev, dtype=torch.float32)
    with eval_mode(model), torch.no_grad():
        if cache is False:
            for s in range(0, n, batch_size):
                e = min(s + batch_size, n)
                scores[s:e] = model.forward_ids(corpus, corpus.sample_user[s:e], corpus.sample_news[s:e].reshape(-1, 1)).reshape(-1)
        else:
            users, uinv = torch.unique(corpus.sample_user, return_inverse=True)
            news, ninv = torch.unique(corpus.sample_news, return_inverse=True)

            def encode(stream_of, rows):
                out = torch.empty((rows.numel(), model.feature_dim), device=dev, dtype=torch.float32)
                for s in range(0, rows.numel(), batch_size):
                    sel = ops.ids32(rows[s:s + batch_size], -1)
                    out[s:s + sel.numel()] = model.towers(stream_of(sel), None)
                return out
            yu = encode(lambda sel: (corpus.user_ids, corpus.user_w, sel), users)
            yn = encode(lambda sel: (corpus.news_ids, corpus.news_w, sel), news)
            for s in range(0, n, batch_size):
                e = min(s + batch_size, n)
                u, v = yu[uinv[s:e]].contiguous(), yn[ninv[s:e]].contiguous()
                logits = torch.empty((e - s, 1), device=dev, dtype=torch.float32)
                ops.cosine_loss(u, v, e - s, 1, model.feature_dim, logits)
                scores[s:e] = logits.reshape(-1)
    return scores
