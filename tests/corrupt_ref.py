"""Test-side reference of message corruption (-bit_flip -corrupt_region, model.py:813-820): the CPU oracle's eval pass
(oracle/cpu_ref.eval_batch) with the Sender's output replaced by |z - m| at every step, m the [W] 0/1 mask broadcast over the
batch.  The oracle itself is not edited: the wrapper sits on the sender module of the agents it is handed."""
import torch

from oracle import cpu_ref


def corrupt_sender(sender, mask):
    """Make `sender` return (|z - m|, probs): what exchange() feeds the Receiver and returns as sen_feats when corrupt=True.
    The probabilities stay the Sender's own."""
    m = torch.as_tensor(mask, dtype=torch.float32).view(1, -1)
    forward = sender.forward

    def corrupted(*args, **kw):
        z, p = forward(*args, **kw)
        return (z - m.expand_as(z)).abs(), p
    sender.forward = corrupted
    return sender


def eval_batch(models, x, target, desc, flags, mask, top_k=None):
    """cpu_ref.eval_batch with the sender's messages corrupted by `mask` (None: uncorrupted)."""
    if mask is not None:
        models = dict(models)
        corrupt_sender(models["sender"], mask)
    return cpu_ref.eval_batch(models, x, target, desc, flags, top_k=top_k)
