"""Host mirror of the reference's ``EmbedAggregator`` (src_seq/farnn/bert_embeddings.py:46-127): a token's rule-space vector
from its word's row of V_embed and an embedding of the token, static or contextual,

    agg = V_embed[w] * beta + nl_add(emb @ embed_r_generalized) * (1 - beta)

-- the input of FARNN_S_SF.  Plain torch on whatever device the tensors live on: the hot path is behind it, in the library.
The reference constructs a BertModel here under --use_bert; this mirror takes the encoder as an argument instead.
"""
import numpy as np
import torch


class EmbedAggregator:
    def __init__(self, args, V, word_embed, encoder=None):
        """encoder: any callable (bert_input, bert_attend_mask, bert_valid_mask, lengths) -> [B, L, D] (forward_bert)."""
        self.args = args
        self.V_embed = torch.from_numpy(np.asarray(V)).float()                         # V x R
        self.V, self.R = self.V_embed.shape
        self.static_embed = torch.from_numpy(np.asarray(word_embed)).float()           # V x D
        self.encoder = encoder
        self.embed_r_generalized = torch.matmul(self.static_embed.pinverse(), self.V_embed)      # D x R (ref :63-66)
        self.beta = args.beta
        self.beta_vec = torch.tensor([self.beta] * self.R).float()
        if args.random:
            torch.nn.init.xavier_normal_(self.V_embed)
            torch.nn.init.xavier_normal_(self.embed_r_generalized)

    def to(self, device):
        for k in ('V_embed', 'static_embed', 'embed_r_generalized', 'beta_vec'):
            setattr(self, k, getattr(self, k).to(device))
        return self

    # ---- training: the leaves behind FARNN_S_SF's d loss / d input ----------------------------------------
    _TRAIN_FLAGS = {'V_embed': 'train_V_embed', 'embed_r_generalized': None, 'beta_vec': 'train_beta'}     # ref :50, :66, :69-71

    def requires_grad_(self, mode=True):
        """Make V_embed, embed_r_generalized and beta_vec autograd leaves with the reference's requires_grad flags (mode=False:
        none of them).  Call it after to(device): the leaves are the tensors where they then live."""
        for k, flag in self._TRAIN_FLAGS.items():
            want = bool(mode) and (flag is None or bool(getattr(self.args, flag, 0)))
            setattr(self, k, getattr(self, k).detach().requires_grad_(want))
        return self

    def named_parameters(self):
        named = [(k, getattr(self, k)) for k in self._TRAIN_FLAGS if getattr(self, k).requires_grad]
        if isinstance(self.encoder, torch.nn.Module):
            named += [('encoder.' + k, t) for k, t in self.encoder.named_parameters() if t.requires_grad]
        return iter(named)

    def parameters(self):
        """The trainable leaves (after requires_grad_()) and, where the encoder is a torch.nn.Module, its parameters."""
        return iter([t for _, t in self.named_parameters()])

    def get_generalized_v_embed_vec(self, v_batch_vec, emb_batch_vec):
        """ref :77-93"""
        gen = torch.einsum('bld,dr->blr', emb_batch_vec.float(), self.embed_r_generalized)
        nl = self.args.additional_nonlinear
        if nl == 'relu':
            gen = torch.relu(gen)
        elif nl == 'tanh':
            gen = torch.tanh(gen)
        elif nl == 'sigmoid':
            gen = torch.sigmoid(gen)
        elif nl == 'relutanh':
            gen = torch.tanh(torch.relu(gen))
        return v_batch_vec * self.beta_vec + gen * (1 - self.beta_vec)

    def _clip(self, inp, lengths):
        L = int(lengths.max().item())
        return inp[:, :L] if L < inp.shape[1] else inp

    def forward(self, inp, lengths):
        """Static word embeddings (ref :95-106): [B, L] word ids -> [B, lengths.max(), R]."""
        inp = self._clip(inp, lengths).to(self.V_embed.device)
        return self.get_generalized_v_embed_vec(self.V_embed[inp], self.static_embed[inp])

    __call__ = forward

    def forward_bert(self, inp, bert_input, bert_attend_mask, bert_valid_mask, lengths):
        """Contextual embeddings (ref :108-128) from ``encoder``."""
        if self.encoder is None:
            raise ValueError('EmbedAggregator.forward_bert needs an encoder: EmbedAggregator(..., encoder=callable)')
        inp = self._clip(inp, lengths).to(self.V_embed.device)
        emb = self.encoder(bert_input, bert_attend_mask, bert_valid_mask, lengths)
        return self.get_generalized_v_embed_vec(self.V_embed[inp], emb.to(self.V_embed.device))
