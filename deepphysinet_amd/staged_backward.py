"""The backward pass of one PDE step, cut where a bucket of gradients is complete (PhysicsNet.gradient_buckets: point statics |
hyper-network heads | encoder layers, norm, projection | data embedding), so that a data-parallel caller can queue that bucket's all-reduce
while the rest of the backward runs.  InterfacePhysics.training_step and StagedPdeStep both cut here; they differ in their forward and in
which cuts share a collective.  Plain torch.autograd.grad calls on whatever tensors the caller hands in: nothing here touches the HIP
library, synchronises or allocates on a side stream, so every cut can be captured into a hipGraph.
"""
import torch


class StagedBackward:
    """buckets: the four parameter lists; placer: an object whose place_gradients(params, grads) puts each gradient where the bucket's
    all-reduce reads it (optim.FusedClipAdam).  The cuts, in order: points, heads -> buckets 0..1 complete; encoder -> bucket 2 (without a
    usable x0: 2..3) complete; embedding -> bucket 3 complete, and every tensor held here released."""
    HELD = ('heads', 'evec', 'meta_out', 'x0', 'g_heads', 'g_evec', 'g_meta', 'g_x0')

    def __init__(self, buckets, placer):
        self.buckets, self.placer = buckets, placer
        self.release()

    def release(self):
        for name in self.HELD:
            setattr(self, name, None)

    def points(self, loss, heads, evec, statics, meta_out, x0, seed):
        """loss -> heads, evec and the statics (bucket 0).  x0: the data embedding's output, the cut between the encoder stack and the
        embedding; None, or one that does not require grad: the encoder cut takes the embedding along."""
        self.heads, self.evec, self.meta_out = heads, evec, meta_out
        self.x0 = x0 if (x0 is not None and x0.requires_grad) else None
        g = torch.autograd.grad(loss, [heads, evec] + list(statics), grad_outputs=seed)
        self.g_heads, self.g_evec = g[0], g[1]
        self.placer.place_gradients(list(statics), g[2:])

    def heads_cut(self):
        params = self.buckets[1]
        g = torch.autograd.grad([self.heads, self.evec], [self.meta_out] + params, grad_outputs=[self.g_heads, self.g_evec], allow_unused=True)
        self.g_meta = g[0]
        self.placer.place_gradients(params, g[1:])

    def encoder(self):
        if self.x0 is None:                                          # no cut available: the whole encoder here, the embedding cut is empty
            params = self.buckets[2] + self.buckets[3]
            g = torch.autograd.grad([self.meta_out], params, grad_outputs=[self.g_meta], allow_unused=True)
            self.placer.place_gradients(params, g)
            return
        params = self.buckets[2]
        g = torch.autograd.grad([self.meta_out], [self.x0] + params, grad_outputs=[self.g_meta], allow_unused=True)
        self.g_x0 = g[0]
        self.placer.place_gradients(params, g[1:])

    def embedding(self):
        if self.g_x0 is not None:
            params = self.buckets[3]
            g = torch.autograd.grad([self.x0], params, grad_outputs=[self.g_x0], allow_unused=True)
            self.placer.place_gradients(params, g)
        self.release()
