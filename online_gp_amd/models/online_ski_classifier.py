"""OnlineSKIClassifier -- Dirichlet-transformed WISKI classifier (two classes by default) (counterpart of
online_gp/models/online_ski_classifier.py:14-145 and gp_dirichlet_classification.py:5-45):

    OnlineSKIClassifier(stem, init_x, init_y, alpha_eps, lr, grid_size, grid_bound, **kw)
    .fit(x, y, num_epochs, test_dataset=None)   .update(x, y, update_stem=True, update_gp=True)   .predict(x) -> labels
    .set_train_data(features, targets, noise)   .set_lr(...)

Labels y in {0, 1} become two regression outputs with heteroscedastic fixed noise: alpha = alpha_eps + onehot(y),
sigma2_i = log(1/alpha + 1), target = log(alpha) - sigma2_i / 2; the predicted class is the argmax of the two posterior
means.  Exercises the 2-output batch layout and non-unit noise of the GP core; the streaming protocol is shared with
the regression wrapper (``_streaming_wrapper.StreamingSKIWrapper``).

``num_classes=C`` gives the same encoding C outputs.  ``likelihood="probit"`` replaces the encoding by the multinomial probit
likelihood of the GP core: ``update`` absorbs the labels themselves through
``condition_on_observations(labels=)``, ``predict_proba`` returns calibrated class probabilities [n, C] with the posterior's error
bars inside, and ``predict`` is their argmax.  The sites of a label depend on the posterior they were matched against, so there
is no closed-form marginal likelihood of labels to train the stem or the hyper-parameters on: ``fit`` and ``update`` with
``update_stem`` / ``update_gp`` raise NotImplementedError on that path."""
import torch

from .. import settings
from ._streaming_wrapper import StreamingSKIWrapper
from .batched_fixed_noise_online_gp import FixedNoiseOnlineSKIGP


def dirichlet_transform(targets, alpha_eps, num_classes=2):
    """labels [n] -> (regression targets [n, C], alpha [n, C], per-point noise variances [n, C])"""
    labels = targets.reshape(-1).long()
    alpha = torch.full((labels.shape[0], num_classes), float(alpha_eps), device=labels.device)
    alpha.scatter_add_(1, labels[:, None], torch.ones_like(alpha[:, :1]))
    sigma2 = torch.log1p(1.0 / alpha)
    return alpha.log() - 0.5 * sigma2, alpha, sigma2


class OnlineSKIClassifier(StreamingSKIWrapper):
    _VOID_NOISE = 1e6         # probit: the noise the first points are created with, so that they say nothing before their labels are absorbed

    def __init__(self, stem, init_x, init_y, alpha_eps, lr, grid_size, grid_bound, num_classes=2, likelihood="dirichlet", **kwargs):
        super().__init__()
        if likelihood not in ("dirichlet", "probit"):
            raise ValueError(f"likelihood must be 'dirichlet' or 'probit', got {likelihood!r}")
        if isinstance(num_classes, bool) or int(num_classes) != num_classes or int(num_classes) < 2:
            raise ValueError(f"num_classes must be an integer >= 2, got {num_classes!r}")
        self.alpha_eps = alpha_eps
        self.num_classes = int(num_classes)
        self.likelihood_kind = likelihood
        self._target_batch_shape = torch.Size([self.num_classes])
        stem = stem.to(init_x.device)
        feats = stem(init_x).detach()
        if likelihood == "probit":
            # the GP core is created from points; these carry no information (zero targets at a noise of 1e6), and their labels are
            # absorbed right below, through the form every later batch takes
            gp_targets = torch.zeros((feats.shape[0], self.num_classes), device=feats.device)
            noise = torch.full_like(gp_targets, self._VOID_NOISE)
        else:
            gp_targets, noise = self._encode(init_y)
        gp = FixedNoiseOnlineSKIGP(feats, gp_targets.to(feats.dtype), noise.to(feats.dtype),
                                   grid_bounds=torch.tensor([[-grid_bound, grid_bound]] * stem.output_dim),
                                   grid_size=[grid_size] * stem.output_dim, forgetting_factor=kwargs.get("forgetting_factor"),
                                   grow_grid=kwargs.get("grow_grid", False), max_grid_size=kwargs.get("max_grid_size"))
        self._setup(stem, gp, lr, init_x)
        if likelihood == "probit":
            with torch.no_grad():
                self._absorb_labels(feats, init_y)
            self._ensure_eval()

    # ----- hooks of the streaming protocol
    def _encode(self, targets):
        gp_targets, _, sigma2 = dirichlet_transform(targets, self.alpha_eps, self.num_classes)
        return gp_targets, sigma2

    def _transform_targets(self, targets, alpha_eps):
        return dirichlet_transform(targets, alpha_eps, self.num_classes)

    def _partial_mll_targets(self, gp_targets, noise):
        return (gp_targets / noise).transpose(-1, -2)            # y / sigma2_i per output

    # ----- the probit path
    def _refuse_training(self, what):
        raise NotImplementedError(f"likelihood='probit': {what} -- the pseudo-observations of a label depend on the posterior they were "
                                  "matched against, so there is no marginal likelihood of the labels to differentiate; absorb with "
                                  "update(x, y, update_stem=False, update_gp=False), or train with likelihood='dirichlet'")

    def _absorb_labels(self, feats, labels):
        self.gp.condition_on_observations(feats, None, labels=labels.reshape(-1).to(feats.device, feats.dtype), inplace=True)

    def update(self, inputs, targets, update_stem=True, update_gp=True):
        if self.likelihood_kind != "probit":
            return super().update(inputs, targets, update_stem=update_stem, update_gp=update_gp)
        if update_stem or update_gp:
            self._refuse_training("update trains neither the stem nor the hyper-parameters on labels")
        with torch.no_grad():
            self._absorb_labels(self.stem(self._as_rows(inputs)), targets)      # (grow_grid: the model follows the features itself)
        self._ensure_eval()
        return 0.0, 0.0

    def predict_proba(self, inputs):
        """P(class | x) [n, C] (float64).  Probit: the multinomial probit probabilities under the posterior
        (``FixedNoiseOnlineSKIGP.label_probability``).  Dirichlet: not available -- the encoding has no calibrated probability."""
        if self.likelihood_kind != "probit":
            raise NotImplementedError("predict_proba needs likelihood='probit': the Dirichlet encoding predicts the argmax of its means only")
        self.eval()
        with torch.no_grad():
            return self.gp.label_probability(self.stem(self._as_rows(inputs)))

    # ----- prediction / training
    def predict(self, inputs):
        if self.likelihood_kind == "probit":
            return self.predict_proba(inputs).argmax(1)
        self.eval()
        with settings.skip_posterior_variances(True):
            return self(inputs).mean.argmax(0)

    def set_train_data(self, inputs, targets, noise):
        if self.likelihood_kind == "probit":
            self._refuse_training("set_train_data rebuilds the statistics from regression targets")
        self.gp.set_train_data(inputs.detach(), targets, noise)

    def fit(self, inputs, targets, num_epochs, test_dataset=None):
        if self.likelihood_kind == "probit":
            self._refuse_training("fit trains the stem and the hyper-parameters jointly")

        def after_epoch():
            acc = float("nan")
            if test_dataset is not None:
                test_x, test_y = test_dataset[:]
                acc = float(self.predict(test_x).eq(test_y.reshape(-1)).float().mean())
            return {"test_acc": acc}

        return self._fit_loop(inputs, targets, num_epochs, after_epoch)
