"""A model wrapper that counts evaluations the way the reference's `eval_fun` does (src/CaNNOLeS.jl:559: neval_residual + neval_cons):
one per residual evaluation and, when the model has constraints, one per constraint evaluation.  outer_loop.solve reads `neval` for its
max_eval test; the lockstep loop's `neval` output is compared with it."""


class CountingModel:
    def __init__(self, model):
        self._model = model
        self.neval = 0

    def __getattr__(self, name):   # structure arrays, sizes, x0 and the derivative callbacks are the wrapped model's
        return getattr(self._model, name)

    def residual(self, x):
        self.neval += 1
        return self._model.residual(x)

    def cons(self, x):
        if self._model.ncon > 0:
            self.neval += 1
        return self._model.cons(x)
