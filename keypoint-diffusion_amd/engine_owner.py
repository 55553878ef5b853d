"""What the four engine-owning modules (the two denoisers, the two keypoint encoders) share: the inference engine that follows the
module's weights, the lazily built training engine, and the protocol of their `torch.autograd.Function`s.

A module lists `EngineOwner` before `nn.Module` and provides `_build_engine()` and `_build_trainer()`.
"""
from . import hip


class EngineOwner:
    _engine = None
    _engine_key = None
    _train = None
    _gemm_mode_hint = ''       # the denoisers (the modules with a `gemm_mode`): what their f16x2 mode needs, for the error below

    def _trainer(self):
        """The training engine and the parameter names in `self.parameters()` order (reference state-dict names)."""
        if self._train is None:
            self._train = (self._build_trainer(), [n for n, _ in self.named_parameters()])
        return self._train

    def _weights_key(self):
        """(storage pointer, version counter) of every parameter: changes when weights are replaced or modified in place.
        Walking the module tree costs ~0.7 ms of host time (hundreds of tensors), more than a B = 1 reverse step takes on the GPU,
        so the list of Parameter objects is cached.  It is rebuilt after `.to()` / `load_state_dict` and whenever ANY module of the
        process registered a parameter since it was built (`hip.param_generation`: `module.weight = nn.Parameter(...)`, parametrize
        and pruning all go through `register_parameter`), so a Parameter object swapped in deep inside the module is seen by the
        next forward.  Unsupported as an immediate trigger: writes into `module._parameters` that bypass `register_parameter` (seen by
        the periodic re-walk below)."""
        gen = hip.param_generation()
        ps = self.__dict__.get('_param_list')
        # every 256th call walks the tree again whatever the hook said: mutations that bypass `register_parameter` (a direct
        # `module._parameters[name] = p`, `__setstate__` / deepcopy swaps) are then seen after at most 256 forwards instead of never
        n = self.__dict__['_param_calls'] = self.__dict__.get('_param_calls', 0) + 1
        if ps is None or self.__dict__.get('_param_gen') != gen or (n & 255) == 0:
            ps = self.__dict__['_param_list'] = list(self.parameters())
            self.__dict__['_param_gen'] = gen
        return tuple([(p.data_ptr(), p._version) for p in ps])

    def _apply(self, fn, *a, **kw):
        self.__dict__.pop('_param_list', None)
        return super()._apply(fn, *a, **kw)

    def load_state_dict(self, *a, **kw):
        self.__dict__.pop('_param_list', None)
        return super().load_state_dict(*a, **kw)

    def engine(self):
        """(Re)build the device engine when weights were replaced or modified in place."""
        key = self._weights_key()
        if self._engine is None or key != self._engine_key:
            eng = self._build_engine()
            eng.load_state_dict(self.state_dict())
            self._engine, self._engine_key = eng, key
        mode = getattr(self, 'gemm_mode', None)                   # the two denoisers have one
        if mode is not None and getattr(self._engine, '_mode_applied', None) != mode:
            if mode not in ('f32', 'f16x2'):
                raise ValueError(f"gemm_mode must be None, 'f32' or 'f16x2', got {mode!r}")
            self._engine.set_gemm_mode(mode)                      # (one library call per engine and choice, not per forward)
            if self._engine.gemm_mode() != mode:                  # an explicit choice is never dropped silently
                raise hip.KpdError(f'gemm_mode={mode!r} was requested but the engine runs {self._engine.gemm_mode()!r} '
                                   f'{self._gemm_mode_hint}')
            self._engine._mode_applied = mode
        return self._engine


def train_forward(ctx, module, params):
    """Head of a training `Function.forward`: the module's trainer with `params` bound for a forward call (no gradient buffers).
    The trainer keeps the saved states of ONE forward.  Every forward takes a new generation number; backward refuses to run on a
    workspace a later forward has overwritten.  The parameters go through save_for_backward, so autograd's version check catches
    an in-place update between forward and backward (the C side reads them in place)."""
    trainer, names = module._trainer()
    ctx.trainer, ctx.names = trainer, names
    trainer.generation = getattr(trainer, 'generation', 0) + 1
    ctx.generation = trainer.generation
    ctx.save_for_backward(*params)
    trainer.bind(names, params, [None] * len(params))
    return trainer


def train_backward(ctx, first: int, module_name: str, states: str):
    """Head of a training `Function.backward`: the parameters (inputs `first` onwards of the forward) bound with zeroed gradient
    buffers for those autograd wants; returns the buffers (None for the others)."""
    if ctx.generation != ctx.trainer.generation:
        raise hip.KpdError(f'backward of a {module_name} forward whose saved {states} were overwritten by a later grad-enabled '
                           f'forward of the same module (one forward/backward pair at a time per module)')
    params = ctx.saved_tensors
    grads = hip.zero_grads_like(params, ctx.needs_input_grad[first:])
    ctx.trainer.bind(ctx.names, params, grads)
    return grads
