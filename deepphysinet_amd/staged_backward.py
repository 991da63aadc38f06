"""The backward pass of one PDE step, cut where a bucket of gradients is complete (PhysicsNet.gradient_buckets: point statics |
hyper-network heads | encoder layers, norm, projection | data embedding), so that a data-parallel caller can queue that bucket's all-reduce
while the rest of the backward runs.  InterfacePhysics.training_step and StagedPdeStep both cut here; they differ in their forward and in
which cuts share a collective.  Plain torch.autograd.grad calls on whatever tensors the caller hands in: nothing here touches the HIP
library, synchronises or allocates on a side stream, so every cut can be captured into a hipGraph.

Frozen parameters (fine-tuning): every cut differentiates only with respect to tensors that require grad.  The buckets handed in are already
filtered to the trainable parameters (a bucket may be empty); with the whole encoder frozen meta_out does not require grad, heads_cut asks for
the heads' parameters alone and the encoder and embedding cuts launch nothing.
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
        self.heads, self.evec = (heads, evec) if heads.requires_grad else (None, None)      # (one node makes both: they require grad together)
        self.meta_out = meta_out if (meta_out is not None and meta_out.requires_grad) else None
        self.x0 = x0 if (x0 is not None and x0.requires_grad) else None
        statics = [p for p in statics if p.requires_grad]          # the point kernels form every static's gradient; a frozen one's is dropped
        cut = [heads, evec] if self.heads is not None else []
        if not cut and not statics:
            return
        g = torch.autograd.grad(loss, cut + statics, grad_outputs=seed)
        if cut:
            self.g_heads, self.g_evec = g[0], g[1]
        self.placer.place_gradients(statics, g[len(cut):])

    def heads_cut(self):
        if self.heads is None:                                       # heads and encoder frozen: nothing behind the point backward
            return
        params = [p for p in self.buckets[1] if p.requires_grad]
        cut = [self.meta_out] if self.meta_out is not None else []
        if not cut and not params:
            return
        g = torch.autograd.grad([self.heads, self.evec], cut + params, grad_outputs=[self.g_heads, self.g_evec], allow_unused=True)
        self.g_meta = g[0] if cut else None
        self.placer.place_gradients(params, g[len(cut):])

    def encoder(self):
        if self.g_meta is None:                                      # the encoder is frozen (or unused): its backward does not run
            return
        if self.x0 is None:                                          # no cut available: the whole encoder here, the embedding cut is empty
            params = [p for p in self.buckets[2] + self.buckets[3] if p.requires_grad]
            g = torch.autograd.grad([self.meta_out], params, grad_outputs=[self.g_meta], allow_unused=True)
            self.placer.place_gradients(params, g)
            return
        params = [p for p in self.buckets[2] if p.requires_grad]
        g = torch.autograd.grad([self.meta_out], [self.x0] + params, grad_outputs=[self.g_meta], allow_unused=True)
        self.g_x0 = g[0]
        self.placer.place_gradients(params, g[1:])

    def embedding(self):
        if self.g_x0 is not None:
            params = [p for p in self.buckets[3] if p.requires_grad]
            g = torch.autograd.grad([self.x0], params, grad_outputs=[self.g_x0], allow_unused=True)
            self.placer.place_gradients(params, g)
        self.release()
