"""Flat-arena Adam: every parameter of a group lives in ONE fp32 buffer (and its gradient in another),
so the optimizer step is a single HIP launch (s2e_adam_flat) and the data-parallel gradient exchange is
an all-reduce over contiguous slices with no packing.  Mirrors torch.optim.Adam as the reference
configures it (models/pix2pix_model.py:92-110): TTUR betas (0, 0.9), eps 1e-8, weight_decay 0."""
import bisect
import os

import torch

from . import ops

_ALIGN = 4          # elements; keeps every parameter 16-byte aligned inside the arena
_ALIGN_CL = 64      # elements; channels-last conv weights start on 256-byte boundaries (see FlatAdam.__init__)
# S2E_WEIGHTS_CL=0: every parameter keeps torch's (Cout, Cin, KH, KW) memory order in the arenas (A/B switch)
_WEIGHTS_CL = os.environ.get('S2E_WEIGHTS_CL', '1') != '0'


def _arena_view(flat, off, p, cl):
    """The parameter-shaped view of its arena slice: plain, or -- conv weights, cl -- the (Cout, Cin, KH, KW) view of a slice
    stored [Cout][KH][KW][Cin] (torch's channels_last): same values, same logical shape, other strides."""
    t = flat[off:off + p.numel()]
    if cl:
        co, ci, kh, kw = p.shape
        return t.view(co, kh, kw, ci).permute(0, 3, 1, 2)
    return t.view(p.shape)


class FlatAdam:
    def __init__(self, params, lr, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0, never_updated=(), channels_last=None,
                 ema_decay=None, ema_start=0, clip_norm=None, skip_nonfinite=False):
        """channels_last (default: on, S2E_WEIGHTS_CL): a conv weight whose input-channel count is a multiple of 8 is stored
        [Cout][KH][KW][Cin] in the arenas -- the order the MFMA kernels' packed matrices and weight gradients use -- and exposed
        as a (Cout, Cin, KH, KW) view: state_dict values, shapes and every element-wise use are unchanged, while the
        weight-gradient kernels accumulate straight into `.grad` and the packs read rows instead of gathering.
        never_updated: parameters that are in the optimizer but never receive a gradient (netE.fc_var: `logvar` enters no
        loss, pix2pix_model.py:307-314).  torch.optim.Adam SKIPS a parameter whose .grad is None -- no moment update and, what
        matters, no weight decay -- so they are laid out at the END of the arenas and the Adam launch stops before them.
        ema_decay (default None: off, nothing is allocated and step() is the plain launch): keep an exponential moving average of
        the parameters in a fifth arena `flat_ema`, updated by the Adam launch itself (s2e_adam_flat_ema: 8 more bytes per
        parameter, no second pass over p).  It starts as a copy of flat_p -- so the never-updated tail holds its parameters from
        the first moment on --; step t (1-based, this optimizer's own count) copies p into it while t <= ema_start and averages
        afterwards, ema = decay * ema + (1 - decay) * p.  `ema_views()` are the per-parameter views.
        clip_norm / skip_nonfinite (default None / False: off, nothing is allocated and step() is the launch it is without them): the
        gradient guard.  step() first examines the active gradient arena (ops.grad_guard: its norm times grad_scale, the first non-finite
        element) and the Adam launch then reads the coefficient from device memory: 0 -- skip_nonfinite and a non-finite element -- leaves
        parameters, moments, the average and the step count alone; min(1, clip_norm / (norm + 1e-6)) scales the gradient as
        torch.nn.utils.clip_grad_norm_ would.  No host round trip per step: `guard_stats()` reads the record when asked."""
        skip = {id(p) for p in never_updated}
        seen, plist = set(), []
        for p in list(params) + [p for p in never_updated]:
            if id(p) not in seen and id(p) not in skip:
                seen.add(id(p))
                plist.append(p)
        n_active_params = len(plist)
        for p in never_updated:
            if id(p) not in seen:
                seen.add(id(p))
                plist.append(p)
        if not plist:
            raise ValueError('FlatAdam got an empty parameter list')
        dev = plist[0].device
        use_cl = _WEIGHTS_CL if channels_last is None else bool(channels_last)
        # (by default only for parameters on the GPU -- the layout exists for the HIP kernels; an explicit True lays out CPU tensors too)
        self.cl = [bool(use_cl and p.dim() == 4 and p.shape[1] % 8 == 0 and (p.is_cuda or channels_last is True)) for p in plist]
        self.offsets, n = [], 0
        for p, cl in zip(plist, self.cl):
            if p.dtype != torch.float32:
                raise TypeError('FlatAdam keeps fp32 master parameters')
            if cl and n % _ALIGN_CL:
                # a channels-last weight starts on a 256-byte boundary: its gradient is the target of the weight-gradient
                # kernels' 128-byte row-segment atomics, which cost per cache line touched (measured +25 % on the 16-byte-aligned
                # slices).  Stacked weights ([W_gamma; W_beta]: sizes are multiples of 64 elements) stay back to back.
                n = (n + _ALIGN_CL - 1) // _ALIGN_CL * _ALIGN_CL
            self.offsets.append(n)
            n += (p.numel() + _ALIGN - 1) // _ALIGN * _ALIGN
        self.numel = n
        self.numel_active = self.offsets[n_active_params] if n_active_params < len(plist) else n
        self.flat_p = torch.zeros(n, dtype=torch.float32, device=dev)
        self.flat_g = torch.zeros(n, dtype=torch.float32, device=dev)
        self.flat_m = torch.zeros(n, dtype=torch.float32, device=dev)
        self.flat_v = torch.zeros(n, dtype=torch.float32, device=dev)
        with torch.no_grad():
            for p, off, cl in zip(plist, self.offsets, self.cl):
                view = _arena_view(self.flat_p, off, p, cl)
                view.copy_(p.data)
                p.data = view                                           # parameter now aliases the arena
                p.grad = _arena_view(self.flat_g, off, p, cl)           # autograd accumulates in place
        self.params = plist
        self._grad_strides = [p.grad.stride() for p in plist]
        self.betas = (float(betas[0]), float(betas[1]))                   # (0, 0.9) must be floats
        self.eps = float(eps)
        self.step_count = 0
        self.param_groups = [{'params': plist, 'lr': float(lr)}]         # update_learning_rate writes ['lr']
        # device-resident hyper-parameters {lr, beta1, beta2, eps, completed steps, grad_scale, weight_decay}
        self._wd = float(weight_decay)
        self.hyper = torch.tensor([float(lr), self.betas[0], self.betas[1], self.eps, 0.0, 1.0, float(weight_decay)],
                                  dtype=torch.float32, device=dev)
        self._hyper_host = (float(lr), 1.0)
        if ema_decay is not None:
            if not 0.0 <= float(ema_decay) < 1.0 or int(ema_start) < 0:
                raise ValueError('FlatAdam: ema_decay must lie in [0, 1) and ema_start must not be negative')
            self.ema_decay, self.ema_start = float(ema_decay), int(ema_start)
            self.flat_ema = self.flat_p.clone()
            # device-resident {decay, start_step}: read by the launch, like `hyper`
            self.ema_hyper = torch.tensor([self.ema_decay, float(self.ema_start)], dtype=torch.float32, device=dev)
        clip = 0.0 if clip_norm is None else float(clip_norm)
        if clip < 0.0:
            raise ValueError('FlatAdam: clip_norm must not be negative')
        if clip > 0.0 or skip_nonfinite:
            self.clip_norm, self.skip_nonfinite = clip, bool(skip_nonfinite)
            # device-resident guard record (seg2eye_hip.h: s2e_grad_guard): {max_norm, skip_nonfinite | norm, coefficient, skipped,
            # clipped, consecutive skips, 0}, the index of the first non-finite element, and the reduction's workspace
            self.guard = torch.tensor([clip, float(self.skip_nonfinite), 0.0, 1.0, 0.0, 0.0, 0.0, 0.0], dtype=torch.float32, device=dev)
            self.first_bad = torch.full((1,), -1, dtype=torch.int32, device=dev)
            self.guard_ws = ops.grad_guard_workspace(self.numel_active, dev)
            self._clip_host = clip

    @property
    def has_ema(self):
        return 'flat_ema' in self.__dict__

    @property
    def has_guard(self):
        return 'guard' in self.__dict__

    def guard_stats(self):
        """The guard record of the last step, by ONE small device-to-host copy (it waits for the stream): {'norm': the gradient's
        norm times grad_scale, 'coef': the coefficient applied (0: skipped), 'skipped' / 'clipped': steps so far, 'consecutive':
        skipped steps in a row, 'first_bad': arena index of the first non-finite element or -1}.  Also sets `step_count` to the
        device's count of COMPLETED steps (hyper[4]): a skipped step is not a step, and only the device knows which were."""
        if not self.has_guard:
            raise RuntimeError('FlatAdam.guard_stats: this optimizer has no gradient guard (clip_norm=None, skip_nonfinite=False)')
        rec = torch.cat([self.guard, self.first_bad.view(torch.float32), self.hyper[4:5]]).cpu()
        self.step_count = int(rec[9])
        return {'norm': float(rec[2]), 'coef': float(rec[3]), 'skipped': int(rec[4]), 'clipped': int(rec[5]), 'consecutive': int(rec[6]),
                'first_bad': int(rec[8:9].view(torch.int32))}

    def param_at(self, flat_index):
        """Position in `params` of the parameter that owns arena element `flat_index` (guard_stats()['first_bad']); None for an
        element of an alignment gap."""
        if not 0 <= flat_index < self.numel:
            raise IndexError('FlatAdam.param_at: %d is outside the arena of %d elements' % (flat_index, self.numel))
        i = bisect.bisect_right(self.offsets, flat_index) - 1
        return i if flat_index < self.offsets[i] + self.params[i].numel() else None

    def ema_views(self):
        """The averaged value of every parameter, in `params` order: views into flat_ema of the parameter's logical shape and --
        channels-last slices included -- strides, exactly as the parameters are views into flat_p."""
        if not self.has_ema:
            raise RuntimeError('FlatAdam.ema_views: this optimizer keeps no average (ema_decay=None)')
        return [_arena_view(self.flat_ema, off, p, cl) for p, off, cl in zip(self.params, self.offsets, self.cl)]

    def swap_ema(self):
        """Exchange the CONTENTS of flat_p and flat_ema (the parameters alias flat_p and captured graphs hold its address, so
        the arenas stay where they are).  Twice = nothing, bit for bit."""
        if not self.has_ema:
            raise RuntimeError('FlatAdam.swap_ema: this optimizer keeps no average (ema_decay=None)')
        with torch.no_grad():
            tmp = self.flat_p.clone()
            self.flat_p.copy_(self.flat_ema)
            self.flat_ema.copy_(tmp)

    def zero_grad(self, set_to_none=False):
        self.flat_g.zero_()
        self._g_is_last_step = False
        ops.ZeroPool.arena_zeroed(self.flat_g)               # (lets the in-place spectral-norm chain rule know the arena is fresh)

    def rebind_grads(self):
        """Re-attach .grad views if something replaced them (e.g. a zero_grad(set_to_none=True))."""
        base, strides = self.flat_g.data_ptr(), self._grad_strides
        for i, p in enumerate(self.params):
            g = p.grad
            if g is not None and g.data_ptr() == base + 4 * self.offsets[i] and g.stride() == strides[i]:
                continue                                     # (the common case, checked without building a view per parameter)
            want = _arena_view(self.flat_g, self.offsets[i], p, self.cl[i])
            if g is not None:
                want.copy_(g)
            p.grad = want

    def sync_hyper(self, grad_scale=1.0):
        """Push lr / grad_scale -- and a changed `clip_norm` -- to the device only when they changed (never inside a graph)."""
        cur = (float(self.param_groups[0]['lr']), float(grad_scale))
        if cur != self._hyper_host:
            self.hyper[0:1].fill_(cur[0])
            self.hyper[5:6].fill_(cur[1])
            self._hyper_host = cur
        if self.has_guard and float(self.clip_norm) != self._clip_host:
            self.guard[0:1].fill_(float(self.clip_norm))
            self._clip_host = float(self.clip_norm)

    def step(self, grad_scale=1.0):
        self.rebind_grads()
        self.sync_hyper(grad_scale)
        self.step_count += 1
        k = self.numel_active
        skips_m = self.betas[0] == 0.0 and self._wd == 0.0
        if self.has_guard:
            # (step_count counts this step as done; guard_stats() corrects it when the device skipped some)
            ops.grad_guard(self.flat_g[:k], self.hyper, self.guard, self.first_bad, self.guard_ws)
            if self.has_ema:
                ops.adam_flat_ema_guarded_step(self.flat_p[:k], self.flat_g[:k], self.flat_m[:k], self.flat_v[:k], self.flat_ema[:k],
                                               self.hyper, self.ema_hyper, self.guard, skips_m=skips_m)
            else:
                ops.adam_flat_guarded_step(self.flat_p[:k], self.flat_g[:k], self.flat_m[:k], self.flat_v[:k], self.hyper, self.guard,
                                           skips_m=skips_m)
        elif self.has_ema:
            ops.adam_flat_ema_step(self.flat_p[:k], self.flat_g[:k], self.flat_m[:k], self.flat_v[:k], self.flat_ema[:k], self.hyper,
                                   self.ema_hyper, skips_m=skips_m)
        else:
            ops.adam_flat_step(self.flat_p[:k], self.flat_g[:k], self.flat_m[:k], self.flat_v[:k], self.hyper, skips_m=skips_m)
        self._g_is_last_step = True

    def _layout(self):
        """What the flat moment arrays mean: element i belongs to which parameter, in which memory order.  `shapes` is the
        per-parameter signature in arena order: a state is only ever loaded into an arena whose parameters have the same
        shapes in the same order (a length check alone accepts a permuted parameter list)."""
        return {'offsets': list(self.offsets), 'channels_last': [bool(c) for c in self.cl],
                'shapes': [tuple(int(d) for d in p.shape) for p in self.params]}

    def _first_moment(self, formed=None):
        """The first-moment arena as torch.optim.Adam would hold it.  With beta1 == 0 and no weight decay (the reference's TTUR
        setting) s2e_adam_flat does not touch flat_m -- m_t = g_t * grad_scale exactly, whatever m was -- so it is formed here from
        the gradient arena when that still holds the gradients of the last step (between step() and the next zero_grad()).
        (With beta1 == 0 the saved m never influences a resumed run: the next step overwrites it.)
        Under the gradient guard the launch consumed g * (grad_scale * c), c the guard's coefficient -- formed here by the kernel's
        own fp32 multiply, on the device -- and a SKIPPED last step consumed nothing: m is then not formed (state_dict: m_valid).
        formed: _m_from_last_step()'s answer when the caller already has it (it costs a read of the guard record)."""
        if self.betas[0] == 0.0 and self._wd == 0.0 and self.step_count > 0 and (self._m_from_last_step() if formed is None else formed):
            k = self.numel_active
            m = self.flat_m.clone()
            m[:k] = self.flat_g[:k] * (self.hyper[5] * self.guard[3] if self.has_guard else self._hyper_host[1])
            return m
        return self.flat_m

    def _m_from_last_step(self, stats=None):
        """The gradient arena still holds the gradient the last step consumed: between step() and the next zero_grad(), and -- under
        the guard -- only when that step was not skipped (`stats`: a guard_stats() record just read, else one is read here)."""
        if not self.__dict__.get('_g_is_last_step', False):
            return False
        return not self.has_guard or (stats or self.guard_stats())['coef'] != 0.0

    def state_dict(self):
        """`m_valid`: False when the saved first moment is NOT the optimizer's -- beta1 == 0 / no weight decay steps leave
        flat_m untouched, and outside the window between step() and the next zero_grad() -- or after a step the gradient guard
        skipped -- the gradient it would be formed from is gone.  Harmless for a resume at beta1 == 0 (the next step overwrites m); a run resumed with another beta1 (--no_TTUR: 0.5)
        must not trust an invalid m: load_state_dict then starts it from zeros.
        With an average (ema_decay) the state also carries `ema`, the flat_ema arena in the layout of m and v."""
        # ONE read of the guard record: step_count then follows the device (skipped steps are not steps) and the coefficient says
        # whether the last step consumed the gradient arena
        formed = self._m_from_last_step(self.guard_stats() if self.has_guard else None)
        skipped = self.betas[0] == 0.0 and self._wd == 0.0 and self.step_count > 0
        valid = (not skipped) or formed
        sd = {'step': self.step_count, 'm': self._first_moment(formed), 'v': self.flat_v, 'lr': self.param_groups[0]['lr'], 'layout': self._layout(),
              'm_valid': valid}
        if self.has_ema:
            sd['ema'] = self.flat_ema                        # (same layout as m and v; absent without an average)
        return sd

    def load_state_dict(self, sd, trust_param_order=False):
        """Moments saved by another FlatAdam.  With a `layout` that carries `shapes` the parameter signature must match; the
        memory order (channels-last flags, alignment gaps) may differ and is converted per parameter by logical index.  A state
        WITHOUT a signature (saved before round 5) is loaded only into the identical arena; a state without any layout (saved
        before channels-last masters / with S2E_WEIGHTS_CL=0) only with `trust_param_order=True`: nothing in it says which
        parameter a moment belongs to, and this build orders the generator's arena differently from the builds that wrote such
        states (pix2pix_model.create_optimizers), so a positional load would attach moments to the wrong weights silently."""
        lay = sd.get('layout')
        mine = self._layout()
        if lay is not None:
            lay = {k: ([tuple(x) for x in v] if k == 'shapes' else list(v)) for k, v in lay.items()}
        if lay is not None and 'shapes' in lay:
            if lay['shapes'] != mine['shapes']:
                raise ValueError('FlatAdam.load_state_dict: the saved moments belong to another parameter list (shapes / order '
                                 'differ from this optimizer\'s): refusing a positional load')
            if lay['offsets'] != mine['offsets'] or lay['channels_last'] != mine['channels_last']:
                return self._load_converted(sd, lay['offsets'], lay['channels_last'])
        elif lay is not None:
            if lay != {k: v for k, v in mine.items() if k != 'shapes'}:
                raise ValueError('FlatAdam.load_state_dict: the saved moments were laid out for another arena (parameter order / '
                                 'channels-last weights differ) and carry no parameter signature')
        else:
            if not trust_param_order:
                raise ValueError('FlatAdam.load_state_dict: the state has no layout / parameter signature (saved before '
                                 'channels-last masters or with S2E_WEIGHTS_CL=0); pass trust_param_order=True only if the '
                                 'parameter ORDER of the optimizer that wrote it is known to equal this one\'s')
            if len(sd['m']) != sum((p.numel() + _ALIGN - 1) // _ALIGN * _ALIGN for p in self.params):
                raise ValueError('FlatAdam.load_state_dict: layout-less state of another total length')
            return self._load_torch_order(sd)
        self.step_count = int(sd['step'])
        for flat, key in self._state_arenas(sd):
            flat.copy_(sd[key])
        self._finish_load(sd)

    def _state_arenas(self, sd):
        """(arena, state key) pairs a load fills: m, v and -- when this optimizer keeps an average and the state carries one -- ema
        (a state without `ema` leaves the average as it is)."""
        pairs = [(self.flat_m, 'm'), (self.flat_v, 'v')]
        if self.has_ema and 'ema' in sd:
            pairs.append((self.flat_ema, 'ema'))
        return pairs

    def _finish_load(self, sd):
        if not sd.get('m_valid', True) and not (self.betas[0] == 0.0 and self._wd == 0.0):
            self.flat_m.zero_()                              # (saved by a beta1 == 0 run outside the step window: see state_dict)
        self.step_count = int(sd['step'])
        self.param_groups[0]['lr'] = float(sd['lr'])
        self.hyper[4:5].fill_(float(self.step_count))
        self.sync_hyper(self._hyper_host[1])

    def _load_converted(self, sd, offsets, cl_flags):
        """Same parameters (signature checked by the caller), other memory order: copied per parameter through views."""
        with torch.no_grad():
            for i, p in enumerate(self.params):
                for flat, key in self._state_arenas(sd):
                    src = _arena_view(sd[key].to(flat.device), offsets[i], p, cl_flags[i])
                    _arena_view(flat, self.offsets[i], p, self.cl[i]).copy_(src)
        self._finish_load(sd)

    def _load_torch_order(self, sd):
        """A state dict without 'layout': moments saved when every parameter lay in torch's order, back to back (4-element
        alignment) -- before channels-last masters, or with S2E_WEIGHTS_CL=0.  Copied per parameter BY LOGICAL INDEX through
        the arena views, so channels-last slices and their 256-byte alignment gaps do not matter."""
        off = 0
        with torch.no_grad():
            for i, p in enumerate(self.params):
                n = p.numel()
                for flat, key in self._state_arenas(sd):
                    _arena_view(flat, self.offsets[i], p, self.cl[i]).copy_(sd[key][off:off + n].view(p.shape))
                off += (n + _ALIGN - 1) // _ALIGN * _ALIGN
        self._finish_load(sd)
