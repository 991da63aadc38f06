#!/usr/bin/env python
"""One pass through the point path's VALUE side at the C ABI, for tests/test_gpu_value_fp64.py: pack -> one of the forward entry points (dpn_fwd,
dpn_fwd_ref, dpn_fwd_ref_nets, dpn_fwd_ref_derivs) and, on request, dpn_bwd_points_derivs with g_hxi -> dpn_wgrad -> dpn_wgrad_finish.  The sibling of
tools/wgrad_digest.run_case (whose model cache and seeded streams it shares; that tool and its fixture are untouched), with what the value side needs:
any geometry and coordinates, ref_data, g_hxi, the forward entry point, the kernel override, and out / jac / hess / d3 kept.

Every output sits in a buffer of its own with rows of a sentinel bit pattern behind row n (bytes behind the sized end for the byte buffers), every
input the kernels index by point sits between NaN guards: a read or write past the n points shows as a NaN in a result or as a damaged sentinel.

    python tools/value_digest.py            # on the GPU: SHA-256 of out / jac / hess / d3 of a few cases of the product build, nothing written"""
import contextlib
import ctypes
import hashlib
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, 'tools')):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import wgrad_digest as WD      # noqa: E402

SENTINEL = -3824219            # 0xFFC5A5A5 as int32: a NaN no kernel computes
TAIL_ROWS = 64                 # sentinel rows behind row n of every [n, ...] output
TAIL_BYTES = 4096              # sentinel bytes behind the sized end of saved / operands / partials
GUARD = 256                    # NaN floats in front of and behind every per-point input
ENTRIES = ('fwd', 'ref', 'nets', 'derivs')


class Owned:
    """An fp32 output [n, cols] inside its own buffer of n + TAIL_ROWS rows, all of it the sentinel before the launch."""

    def __init__(self, n, cols, dev):
        import torch
        self.n = n
        self.buf = torch.full(((n + TAIL_ROWS) * cols,), SENTINEL, dtype=torch.int32, device=dev)
        self.rows = self.buf.view(torch.float32).view(n + TAIL_ROWS, cols)

    def read(self):
        """(the n rows on the host, True if every row behind them still holds the sentinel)"""
        import torch
        rows = self.buf.cpu().view(self.n + TAIL_ROWS, -1)
        return rows[:self.n].view(torch.float32).clone(), bool((rows[self.n:] == SENTINEL).all())

    def untouched(self):
        return bool((self.buf == SENTINEL).all())


class OwnedBytes:
    """A byte buffer of `size` zeroed bytes (the kernels leave some unwritten) and TAIL_BYTES of 0xA5 behind them."""

    def __init__(self, size, dev, fill=0):
        import torch
        self.size = int(size)
        self.buf = torch.full((self.size + TAIL_BYTES,), 0xA5, dtype=torch.uint8, device=dev)
        self.buf[:self.size] = fill

    def read(self):
        host = self.buf.cpu()
        return host[:self.size].clone(), bool((host[self.size:] == 0xA5).all())

    def untouched(self, fill=0):
        return bool((self.buf[:self.size] == fill).all()) and bool((self.buf[self.size:] == 0xA5).all())


def guarded(t, dev):
    """t on the device between two runs of GUARD NaNs (the view the launches are handed, the whole buffer)."""
    import torch
    if t is None:
        return None, None
    t = t.to(torch.float32).contiguous()
    buf = torch.full((t.numel() + 2 * GUARD,), float('nan'), dtype=torch.float32, device=dev)
    buf[GUARD:GUARD + t.numel()] = t.reshape(-1).to(dev)
    return buf[GUARD:GUARD + t.numel()].view(t.shape), buf


class Pass:
    """The device side of one case: the model's weights (tools/wgrad_digest._model: oracle fills at `gain`), packed under the kernel choice `fwd_kernel`
    (None: the library's own; 'ring' | 'tiles': DPN_FWD_KERNEL, set around the pack call and every forward launch alike, so that the stream is in the form
    dpn_fwd_form returns for the kernel that reads it), and the guarded inputs.  coords = (x, y, t) [n] host tensors (default: the NCEP synthetic ones),
    geometry = (dx, dy, lon - 1, lat - 1, span) (default: the model's)."""

    def __init__(self, route, n, prec, gain=1.0, geometry=None, coords=None, coord_data=None, ref_data=None, pe_in=None, fwd_kernel=None):
        import torch
        from deepphysinet_amd import _lib as L
        from deepphysinet_amd import point_path as P
        from oracle.fill import synthetic_inputs
        self.L, self.P, self.lib = L, P, L.load()
        self.route, self.n, self.fwd_kernel = route, n, fwd_kernel
        m = WD._model(prec, gain)
        self.dev = dev = torch.device('cuda:0')
        syn = synthetic_inputs(n, tag='inter')
        self.cfg = cfg = m.point_config()
        with torch.no_grad():
            heads, evec, statics = m.physics_net.field_weights(syn['field_data'].to(dev), syn['forecast_h'].to(dev))
        self.heads, self.evec = heads.detach().contiguous(), evec.detach().contiguous()
        self.statics = [s.detach().contiguous() for s in statics]
        self.nets = P._net_ptrs(self.heads, self.evec, self.statics)
        self.geo = cfg.geometry() if geometry is None else L.DpnGeometry(*[float(v) for v in geometry])
        self.geometry = (self.geo.dx, self.geo.dy, self.geo.lon_m1, self.geo.lat_m1, self.geo.pred_t_span)
        x, y, t = (syn[k].reshape(-1) for k in ('x', 'y', 't')) if coords is None else coords
        self.host = dict(x=x, y=y, t=t, coord_data=syn['coord_data'] if coord_data is None else coord_data, ref_data=ref_data,
                         pe_in=pe_in if route == 'pe_in' else None)
        self.d, self.guards = {}, {}
        for k, v in self.host.items():
            self.d[k], self.guards[k] = guarded(v, dev)
        self.fr = P._freqs(dev)
        self.ws = P._Workspace(n, cfg.prec, dev)
        with self._kernel():
            self.form = self.lib.dpn_fwd_form(cfg.prec, 0 if self.d['pe_in'] is None else 1)
            L.check(self.lib.dpn_pack_weights_form(self.nets, cfg.prec, self.form, P._ptr(self.ws.packed), P._stream()), 'pack')

    @contextlib.contextmanager
    def _kernel(self):
        prev = os.environ.get('DPN_FWD_KERNEL')
        if self.fwd_kernel:
            os.environ['DPN_FWD_KERNEL'] = self.fwd_kernel
        try:
            yield
        finally:
            if self.fwd_kernel:
                if prev is None:
                    os.environ.pop('DPN_FWD_KERNEL', None)
                else:
                    os.environ['DPN_FWD_KERNEL'] = prev

    def forward(self, entry='ref', want=('jac', 'hess', 'd3', 'saved'), n_nets=6, **override):
        """One forward launch.  entry: 'fwd' dpn_fwd | 'ref' dpn_fwd_ref | 'nets' dpn_fwd_ref_nets (n_nets) | 'derivs' dpn_fwd_ref_derivs; want: the optional
        outputs that are not NULL (jac never on the pe_in route, hess / d3 only with 'derivs', saved not with 'nets').  override: argument name -> value
        in place of the case's (x, y, t, pe_in, coord_data, ref_data, n, freqs, geo, packed, prec, out_n as raw values; None is NULL) -- for the refusals that
        return before any launch.  Returns {'rc', 'out', 'jac', 'hess', 'd3': Owned or None, 'saved': OwnedBytes or None}; nothing is synchronised."""
        P, lib, n, dev = self.P, self.lib, self.n, self.dev
        raw = self.route == 'raw'
        o = {'out': Owned(n, 6, dev), 'jac': Owned(n, 18, dev) if ('jac' in want and raw) else None,
             'hess': Owned(n, 18, dev) if ('hess' in want and entry == 'derivs') else None, 'd3': Owned(n, 18, dev) if ('d3' in want and entry == 'derivs') else None,
             'saved': OwnedBytes(self.ws.sizes.saved, dev) if ('saved' in want and entry != 'nets') else None}
        ptr = lambda k: None if o[k] is None else P._ptr(o[k].buf)
        a = dict(x=P._ptr(self.d['x']) if raw else None, y=P._ptr(self.d['y']) if raw else None, t=P._ptr(self.d['t']) if raw else None, pe_in=P._ptr(self.d['pe_in']),
                 coord_data=P._ptr(self.d['coord_data']), ref_data=P._ptr(self.d['ref_data']), n=n, freqs=P._ptr(self.fr), geo=ctypes.byref(self.geo),
                 packed=P._ptr(self.ws.packed), prec=self.cfg.prec, out_n=ptr('out'), n_nets=n_nets)
        a.update(override)
        head = (a['x'], a['y'], a['t'], a['pe_in'], a['coord_data'])
        mid = (a['n'], a['freqs'], a['geo'], a['packed'], a['prec'])
        with self._kernel():
            if entry == 'fwd':
                rc = lib.dpn_fwd(*head, *mid, a['out_n'], ptr('jac'), ptr('saved'), P._stream())
            elif entry == 'ref':
                rc = lib.dpn_fwd_ref(*head, a['ref_data'], *mid, a['out_n'], ptr('jac'), ptr('saved'), P._stream())
            elif entry == 'nets':
                rc = lib.dpn_fwd_ref_nets(*head, a['ref_data'], *mid, a['n_nets'], a['out_n'], ptr('jac'), P._stream())
            else:
                rc = lib.dpn_fwd_ref_derivs(*head, a['ref_data'], *mid, a['out_n'], ptr('jac'), ptr('hess'), ptr('d3'), ptr('saved'), P._stream())
        o['rc'] = int(rc)
        return o

    def backward_derivs(self, saved, g_out, g_jxi, g_hxi, scale):
        """dpn_bwd_points_derivs (g_hxi may be None) on the saved state of a forward launch -> dpn_wgrad -> dpn_wgrad_finish.  Cotangents: host tensors.
        Returns {'operands', 'partials': OwnedBytes, 'g_heads', 'g_evec', 'statics', 'k_splits'}."""
        import torch
        L, P, lib, n, dev = self.L, self.P, self.lib, self.n, self.dev
        g_out = g_out.to(dev, torch.float32).contiguous()
        g_jxi = g_jxi.to(dev, torch.float32).contiguous()
        self.host['g_hxi'] = g_hxi
        self.d['g_hxi'], self.guards['g_hxi'] = guarded(g_hxi, dev)
        sc = torch.full((1,), float(scale), device=dev)
        operands, partials = OwnedBytes(self.ws.sizes.operands, dev), OwnedBytes(self.ws.sizes.partials, dev)
        L.check(lib.dpn_bwd_points_derivs(P._ptr(self.d['x']), P._ptr(self.d['y']), P._ptr(self.d['t']), None, P._ptr(self.d['coord_data']), n, P._ptr(self.fr),
                                          ctypes.byref(self.geo), P._ptr(self.ws.packed), self.cfg.prec, P._ptr(g_out), P._ptr(g_jxi), P._ptr(self.d['g_hxi']),
                                          P._ptr(sc), P._ptr(saved.buf), P._ptr(operands.buf), P._stream()), 'bwd derivs')
        g_heads = torch.empty(256, P.HEADS_COLS, device=dev)
        g_evec = torch.empty(6, 256, device=dev)
        g_stat = [torch.empty(P.STATIC_SHAPES[i % 8], device=dev) for i in range(48)]
        L.check(lib.dpn_wgrad(n, self.cfg.prec, P._ptr(g_out), P._ptr(saved.buf), P._ptr(operands.buf), P._ptr(partials.buf), P._stream()), 'wgrad')
        L.check(lib.dpn_wgrad_finish(self.nets, P._ptr(self.ws.packed), n, self.cfg.prec, P._ptr(partials.buf),
                                     P._net_ptrs(g_heads, g_evec, g_stat, cls=L.DpnNetGradPtrs), P._stream()), 'finish')
        return dict(operands=operands, partials=partials, g_heads=g_heads, g_evec=g_evec, statics=g_stat, k_splits=int(self.ws.sizes.k_splits))

    def guards_intact(self):
        """every guard still NaN and every input between them unchanged (the kernels only read them)"""
        import torch
        ok = True
        for k, buf in self.guards.items():
            if buf is None:
                continue
            host = buf.cpu()
            ok = ok and bool(torch.isnan(host[:GUARD]).all()) and bool(torch.isnan(host[-GUARD:]).all())
            ok = ok and torch.equal(host[GUARD:-GUARD], self.host[k].to(torch.float32).reshape(-1))
        return ok


def run_case(route, n, prec, gain=1.0, geometry=None, coords=None, coord_data=None, ref_data=None, pe_in=None, entry='ref', fwd_kernel=None,
             want=('jac', 'hess', 'd3', 'saved'), n_nets=6, cotangents=None, g_hxi=None, scale=WD.G_SCALE):
    """One pass, one synchronisation, one read-back.  Returns host tensors: 'out' [n, 6], 'jac' / 'hess' / 'd3' [n, 6, 3] or None, 'saved' (uint8) or None,
    'tails' {name: the sentinel behind the output survived}, 'guards' (Pass.guards_intact), 'inputs' (heads, evec, statics, geometry, form) and, with
    cotangents = (g_out, g_jxi) [and g_hxi], the weight side behind dpn_bwd_points_derivs: 'operands', 'partials', 'g_heads', 'g_evec', 'statics', 'k_splits'."""
    import torch
    p = Pass(route, n, prec, gain=gain, geometry=geometry, coords=coords, coord_data=coord_data, ref_data=ref_data, pe_in=pe_in, fwd_kernel=fwd_kernel)
    f = p.forward(entry, want=want, n_nets=n_nets)
    p.L.check(f['rc'], entry)
    b = p.backward_derivs(f['saved'], cotangents[0], cotangents[1], g_hxi, scale) if cotangents is not None else None
    torch.cuda.synchronize()
    res, tails = {}, {}
    for k in ('out', 'jac', 'hess', 'd3', 'saved'):
        res[k], tails[k] = (None, True) if f[k] is None else f[k].read()
    for k in ('jac', 'hess', 'd3'):
        if res[k] is not None:
            res[k] = res[k].view(n, 6, 3)
    if b is not None:
        for k in ('operands', 'partials'):
            res[k], tails[k] = b[k].read()
        res.update(g_heads=b['g_heads'].cpu(), g_evec=b['g_evec'].cpu(), statics=[s.cpu() for s in b['statics']], k_splits=b['k_splits'])
    res.update(tails=tails, guards=p.guards_intact(),
               inputs=dict(heads=p.heads.cpu(), evec=p.evec.cpu(), statics=[s.cpu() for s in p.statics], geometry=p.geometry, form=int(p.form)))
    return res


def main():
    for route, n, prec, entry in (('raw', 70, 'bf16x2', 'derivs'), ('raw', 1037, 'bf16x2', 'derivs'), ('raw', 70, 'bf16', 'derivs'), ('pe_in', 70, 'bf16x2', 'ref')):
        import torch
        pe_in = torch.sin(torch.randn(n, 192, generator=torch.Generator().manual_seed(4)) * 3.0) if route == 'pe_in' else None
        res = run_case(route, n, prec, entry=entry, pe_in=pe_in)
        print('%s/%d/%s/%s' % (route, n, prec, entry), ' '.join('%s %s' % (k, hashlib.sha256(res[k].contiguous().numpy().tobytes()).hexdigest()[:16])
                                                                  for k in ('out', 'jac', 'hess', 'd3') if res[k] is not None), flush=True)


if __name__ == '__main__':
    main()
