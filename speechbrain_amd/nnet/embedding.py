"""speechbrain.nnet.embedding mirror."""
import torch


class Embedding(torch.nn.Module):
    """nnet/embedding.py:15-125: holder of the table; the decoder kernels gather from ``Embedding.weight`` directly.

    consider_as_one_hot=True builds the reference's one-hot table (nnet/embedding.py:80-100): [V, V-1], the blank's row zero
    and the other rows the unit vectors in order; a transducer search folds it into its LSTM's input weights."""

    def __init__(self, num_embeddings, embedding_dim=128, consider_as_one_hot=False, blank_id=0):
        super().__init__()
        self.num_embeddings, self.consider_as_one_hot, self.blank_id = num_embeddings, consider_as_one_hot, blank_id
        if consider_as_one_hot:
            self.embedding_dim = num_embeddings - 1
            self.Embedding = torch.nn.Embedding(num_embeddings, self.embedding_dim, padding_idx=blank_id)
            one_hot = torch.eye(self.embedding_dim)
            if blank_id + 1 != num_embeddings:
                self.Embedding.weight.data[blank_id + 1:] = one_hot[blank_id:]
            if blank_id != 0:
                self.Embedding.weight.data[:blank_id] = one_hot[:blank_id]
            self.Embedding.weight.requires_grad = False
        else:
            self.embedding_dim = embedding_dim
            self.Embedding = torch.nn.Embedding(num_embeddings, embedding_dim)
