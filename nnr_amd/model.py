"""`Model(news_encoder, user_encoder, click_predictor)` -- the reference's plugin hub (model.py:10-133) for the
in-scope encoders, dispatching on the same `--news_encoder / --user_encoder` strings; forward takes the same 21
positional tensors (trainer.py:105-106) and returns logits [batch, 1 + negative_sample_num]."""
import torch
import torch.nn as nn

from . import ops
from . import news_encoders as newsEncoders
from . import user_encoders as userEncoders


class _DotProductFn(torch.autograd.Function):
    """logits = (user_representation * news_representation).sum(dim=2)   (model.py:126-127)"""

    @staticmethod
    def forward(ctx, user, cand):
        B, N, D = cand.shape
        user, cand = user.contiguous(), cand.contiguous()
        logits = torch.empty((B, N), device=cand.device, dtype=torch.float32)
        ops.logits_fwd(user, cand, B, N, D, logits)
        ctx.save_for_backward(user, cand)
        return logits

    @staticmethod
    def backward(ctx, dlogits):
        user, cand = ctx.saved_tensors
        B, N, D = cand.shape
        duser, dcand = torch.empty_like(user), torch.empty_like(cand)
        ops.logits_bwd(dlogits.contiguous(), user, cand, B, N, D, duser, dcand)
        return duser, dcand


class _NegLogSoftmaxFn(torch.autograd.Function):
    """loss = (-log_softmax(logits, dim=1)[:, 0]).mean()   (trainer.py:64-66); the gradient is produced in the same pass."""

    @staticmethod
    def forward(ctx, logits):
        B, N = logits.shape
        logits = logits.contiguous()
        loss = torch.empty((), device=logits.device, dtype=torch.float32)
        dlogits = torch.empty_like(logits)
        ops.nls_loss(logits, B, N, loss, dlogits)
        ctx.save_for_backward(dlogits)
        return loss

    @staticmethod
    def backward(ctx, dloss):
        (dlogits,) = ctx.saved_tensors
        return dlogits * dloss


class _JoinSideFn(torch.autograd.Function):
    """Fork/join of the candidate encoder call that ran on a side HIP stream (autograd-based encoders, GPU-bound steps).
    forward: the current (main) stream waits for the side stream.  backward: autograd runs the candidate call's backward nodes
    on the side stream again (and orders them behind the producer of this gradient); the end-of-pass callback joins the side
    stream back, because those nodes write parameter gradients out of autograd's sight."""

    @staticmethod
    def forward(ctx, side, *xs):
        ctx.side, ctx.main = side, torch.cuda.current_stream(xs[0].device)
        ctx.main.wait_stream(side)
        out = tuple(x.view_as(x) for x in xs)        # (a pair for the HDC representation (d0, dL))
        return out[0] if len(out) == 1 else out

    @staticmethod
    def backward(ctx, *gs):
        side = ctx.side
        for g in gs:
            if g is not None:
                g.record_stream(side)                # consumed by side-stream kernels after this node's buffer is released
        dev = next(g.device for g in gs if g is not None)
        torch.autograd.Variable._execution_engine.queue_callback(lambda: ops.join_extra_streams(dev))
        return (None,) + tuple(gs)


def negative_log_softmax(logits):
    return _NegLogSoftmaxFn.apply(logits)


class Model(nn.Module):
    def __init__(self, config, word_table=None, entity_table=None, context_table=None):
        super().__init__()
        if config.news_encoder == 'HDC' or config.user_encoder == 'FIM':
            # model.py:86-88, ahead of the encoders: there the other user encoders fail on HDC's news_embedding_dim = None before these are reached
            assert config.news_encoder == 'HDC' and config.user_encoder == 'FIM', 'HDC and FIM must be paired and can not be used alone'
            assert config.click_predictor == 'FIM', 'For the model FIM, the click predictor must be specially set as \'FIM\''
        if config.news_encoder == 'CNE':
            self.news_encoder = newsEncoders.CNE(config, word_table)
        elif config.news_encoder == 'CNN':
            self.news_encoder = newsEncoders.CNN(config, word_table)
        elif config.news_encoder == 'MHSA':
            self.news_encoder = newsEncoders.MHSA(config, word_table)
        elif config.news_encoder == 'PNE':
            self.news_encoder = newsEncoders.PNE(config, word_table)
        elif config.news_encoder == 'DAE':
            self.news_encoder = newsEncoders.DAE(config, word_table)
        elif config.news_encoder == 'Inception':
            self.news_encoder = newsEncoders.Inception(config, word_table)
        elif config.news_encoder == 'KCNN':
            self.news_encoder = newsEncoders.KCNN(config, word_table, entity_table, context_table)
        elif config.news_encoder == 'HDC':
            self.news_encoder = newsEncoders.HDC(config, word_table)
        elif config.news_encoder == 'NAML_Title':
            self.news_encoder = newsEncoders.NAML_Title(config, word_table)
        elif config.news_encoder == 'NAML_Content':
            self.news_encoder = newsEncoders.NAML_Content(config, word_table)
        elif config.news_encoder in ('CNE_Title', 'CNE_Content', 'CNE_wo_CS', 'CNE_wo_CA'):
            self.news_encoder = getattr(newsEncoders, config.news_encoder)(config, word_table)
        else:
            raise Exception(config.news_encoder + ' is not on the MI355X hot path (in scope: CNE, CNN, MHSA, HDC, PNE, DAE, Inception, KCNN, NAML_Title, '
                            'NAML_Content, CNE_Title, CNE_Content, CNE_wo_CS, CNE_wo_CA; SURVEY.md section 8a; of variantEncoders.py also the user '
                            'encoders SUE_wo_GCN, SUE_wo_HCA)')
        if config.user_encoder == 'SUE':
            self.user_encoder = userEncoders.SUE(self.news_encoder, config)
        elif config.user_encoder == 'MHSA':
            self.user_encoder = userEncoders.MHSA(self.news_encoder, config)
        elif config.user_encoder == 'ATT':
            self.user_encoder = userEncoders.ATT(self.news_encoder, config)
        elif config.user_encoder == 'CATT':
            self.user_encoder = userEncoders.CATT(self.news_encoder, config)
        elif config.user_encoder == 'OMAP':
            self.user_encoder = userEncoders.OMAP(self.news_encoder, config)
        elif config.user_encoder == 'PUE':
            self.user_encoder = userEncoders.PUE(self.news_encoder, config)
        elif config.user_encoder == 'FIM':
            self.user_encoder = userEncoders.FIM(self.news_encoder, config)
        elif config.user_encoder == 'GRU':
            self.user_encoder = userEncoders.GRU(self.news_encoder, config)
        elif config.user_encoder == 'SUE_wo_GCN':
            self.user_encoder = userEncoders.SUE_wo_GCN(self.news_encoder, config)
        elif config.user_encoder == 'SUE_wo_HCA':
            self.user_encoder = userEncoders.SUE_wo_HCA(self.news_encoder, config)
        else:
            raise Exception(config.user_encoder + ' is not on the MI355X hot path (in scope: SUE, MHSA, ATT, CATT, FIM, OMAP, PUE, GRU; SURVEY.md section 8a; '
                            'of variantEncoders.py, beside the news encoders CNE_Title, CNE_Content, CNE_wo_CS, CNE_wo_CA, the ablations SUE_wo_GCN, SUE_wo_HCA)')
        self.model_name = config.news_encoder + '-' + config.user_encoder
        self.news_embedding_dim = self.news_encoder.news_embedding_dim
        self.dropout = nn.Dropout(p=config.dropout_rate)                    # (model.py:77: part of the attribute surface; the user rows'
                                                                              #  dropout is fused into their gather, see forward)
        self.dropout_rate = float(config.dropout_rate)
        # model.py:79-85: the personalised encoders (NPA) read a trainable table indexed by the batch's user_ID.  No padding_idx: row 0
        # receives gradient like any other row.
        self.use_user_embedding = config.news_encoder == 'PNE' or config.user_encoder == 'PUE'
        if self.use_user_embedding:
            self.user_embedding = nn.Embedding(num_embeddings=config.user_num, embedding_dim=config.user_embedding_dim)
            self._user_seed_base = int(getattr(config, 'seed', 0)) * 6151 + 43
            self._user_calls = 0
        if config.click_predictor != ('FIM' if config.user_encoder == 'FIM' else 'dot_product'):
            raise Exception('click_predictor=%s is out of scope (dot_product, and FIM with the HDC / FIM pair; model.py:126-132)' % config.click_predictor)
        self.click_predictor = config.click_predictor
        if self.click_predictor == 'FIM':                                                 # model.py:93-105
            ue = self.user_encoder
            S, H = self.news_encoder.HDC_sequence_length, config.max_history_num
            first = (ue.conv_3D_a.out_channels, ue.conv_3D_a.kernel_size[0])
            second = (ue.conv_3D_b.out_channels, ue.conv_3D_b.kernel_size[0])

            def pooled(size):
                conv1 = size - first[1] + 1
                pool1 = (conv1 - ue.pool_size) // ue.pool_stride + 1
                conv2 = pool1 - second[1] + 1
                return (conv2 - ue.pool_size) // ue.pool_stride + 1
            feature_size = pooled(S) * pooled(S) * pooled(H) * second[0]
            # every limit of the fused layers (csrc/fim.hip), LDS footprint included, here and not at the first forward
            da = ops.conv3d_pool_plan(4, H, S, S, first[0], first[1], ue.pool_size, ue.pool_stride)
            if da is None or ops.conv3d_pool_plan(first[0], da[0], da[1], da[2], second[0], second[1], ue.pool_size, ue.pool_stride) is None:
                raise Exception('HDC-FIM: ' + ops.FIM_UNSUPPORTED)
            self.fc = nn.Linear(in_features=feature_size, out_features=1, bias=True)

    def initialize(self):
        self.news_encoder.initialize()
        self.user_encoder.initialize()
        if self.use_user_embedding:                                         # model.py:110-112
            nn.init.uniform_(self.user_embedding.weight, -0.1, 0.1)
            with torch.no_grad():
                self.user_embedding.weight[0].zero_()
        if self.click_predictor == 'FIM':                                   # model.py:116-118
            nn.init.xavier_uniform_(self.fc.weight)
            nn.init.zeros_(self.fc.bias)

    def user_rows(self, user_ID):
        """dropout(user_embedding(user_ID)) (model.py:122), computed once per forward and handed to both news-encoder calls and to the user
        encoder; None for the encoder pairs that do not read the table."""
        if not self.use_user_embedding:
            return None
        from .functional import UserRowsFn
        self._user_calls += 1
        seed = (self._user_seed_base + 7368787 * self._user_calls) & 0x7FFFFFFF
        return UserRowsFn.apply(self.user_embedding.weight, user_ID, self.dropout_rate if self.training else 0.0, seed)

    def _encode_user(self, user_embedding, *args):
        """encode_user(*args), with the user rows for the encoders that read them: the one place that decides (evaluate.py calls it too)."""
        if self.user_encoder.needs_user_embedding:
            return self.user_encoder.encode_user(*args, user_embedding)
        return self.user_encoder.encode_user(*args)

    def forward(self, user_ID, user_category, user_subCategory, user_title_text, user_title_mask, user_title_entity, user_content_text,
                user_content_mask, user_content_entity, user_history_mask, user_history_graph, user_history_category_mask,
                user_history_category_indices, news_category, news_subCategory, news_title_text, news_title_mask, news_title_entity,
                news_content_text, news_content_mask, news_content_entity):
        user_embedding = self.user_rows(user_ID)
        if self.training and torch.is_grad_enabled() and news_title_text.is_cuda:
            ops.wt_prefetch(news_title_text.device)      # W^T copies the backward pass will want, off the critical chain
        ne = self.news_encoder
        if (hasattr(ne, 'forward_pair') and not self.training and not torch.is_grad_enabled() and news_title_text.is_cuda
                and ne.pad_dedup and ne.tie_order == 'stable' and hasattr(self.user_encoder, 'encode_user')):
            # inference: the history call without its redundant PAD slots (exact; news_encoders.cne_history_dedup)
            news_representation = ne(news_title_text, news_title_mask, news_title_entity, news_content_text, news_content_mask,
                                     news_content_entity, news_category, news_subCategory, user_embedding)
            history_embedding, rows = newsEncoders.cne_history_dedup(ne, user_title_text, user_title_mask, user_content_text, user_content_mask,
                                                                     user_category, user_subCategory)
            st = ne.__dict__.setdefault('_dedup_stats', [0, 0])
            st[0] += rows
            st[1] += user_title_text.shape[0] * user_title_text.shape[1]
            user_representation = self._encode_user(user_embedding, history_embedding, user_history_mask, user_history_graph,
                                                    user_history_category_mask, user_history_category_indices, news_representation)
        elif hasattr(self.news_encoder, 'forward_pair'):
            # same arithmetic as the two encoder calls of model.py:123-125, issued in lock-step so that launch-latency-bound
            # stages (the Bi-LSTM recurrences) of the candidate call and of the history call share one launch
            news_representation, history_embedding = self.news_encoder.forward_pair(
                (news_title_text, news_title_mask, news_content_text, news_content_mask, news_category, news_subCategory),
                (user_title_text, user_title_mask, user_content_text, user_content_mask, user_category, user_subCategory))
            user_representation = self._encode_user(user_embedding, history_embedding, user_history_mask, user_history_graph,
                                                    user_history_category_mask, user_history_category_indices, news_representation)
        else:
            # size class of this step for ops.leaf_deferred: the token rows of the history call
            ops.STEP_ROWS[0] = user_title_text.shape[0] * user_title_text.shape[1] * user_title_text.shape[2]
            cand = (news_title_text, news_title_mask, news_title_entity, news_content_text, news_content_mask, news_content_entity,
                    news_category, news_subCategory, user_embedding)
            if news_title_text.is_cuda and ops.SIDE_CALL and ops.STEP_ROWS[0] >= ops.LEAF_MIN_ROWS and hasattr(self.user_encoder, 'encode_user'):
                # GPU-bound step: the small candidate call runs on a side HIP stream next to the history call (same launches,
                # same seeds, same order of the dropout counters as the sequential form below)
                dev = news_title_text.device
                side, main = newsEncoders._side_stream(dev), torch.cuda.current_stream(dev)
                side.wait_stream(main)
                with torch.cuda.stream(side):
                    news_representation = self.news_encoder(*cand)
                history_embedding = self.news_encoder(user_title_text, user_title_mask, user_title_entity, user_content_text,
                                                      user_content_mask, user_content_entity, user_category, user_subCategory, user_embedding)
                if isinstance(news_representation, tuple):
                    news_representation = _JoinSideFn.apply(side, *news_representation)
                else:
                    news_representation = _JoinSideFn.apply(side, news_representation)
                user_representation = self._encode_user(user_embedding, history_embedding, user_history_mask, user_history_graph,
                                                        user_history_category_mask, user_history_category_indices, news_representation)
            else:
                news_representation = self.news_encoder(*cand)
                user_representation = self.user_encoder(user_title_text, user_title_mask, user_title_entity, user_content_text,
                                                        user_content_mask, user_content_entity, user_category, user_subCategory,
                                                        user_history_mask, user_history_graph, user_history_category_mask,
                                                        user_history_category_indices, user_embedding, news_representation)
        if self.click_predictor == 'FIM':                                   # model.py:131-132
            from .functional import LinearFn
            B, N, D = user_representation.shape
            return LinearFn.apply(user_representation.reshape(B * N, D), self.fc.weight, self.fc.bias, ops.ACT_NONE, 0.0, 0).view(B, N)
        return _DotProductFn.apply(user_representation, news_representation)
