"""Monkey-patch a running CBAS backend so its unmodified worker threads use the MI355X path.

    import cbas_amd.integration; cbas_amd.integration.install()

Replaces ``cbas.DinoEncoder`` / ``cbas.encode_file`` / ``cbas.infer_file`` (reference
backend/cbas.py:399-572, 650-677) and ``classifier_head.ClassifierLSTMDeltas``
(backend/classifier_head.py:57-172) with the drop-ins of this package, and the training path with it:
``cbas.train_lstm_model``, ``cbas.evaluate_on_split`` (cbas.py:1222-1251) and, when the ``workthreads`` module can be
imported, ``workthreads.fit_temperature`` (workthreads.py:103-137) and ``TrainingThread._execute_training_task``, which
is run inside ``cbas_amd.train.keep_rows()`` so that the runs, trials, test split and calibration of one training job
share one store of CLS rows in device memory.  ``install(postprocess=True)`` also replaces what CBAS does with the
probabilities afterwards - ``cbas.Dataset.predictions_to_instances`` / ``predictions_to_instances_with_confidence``
(cbas.py:903-956) and the activity behind ``cbas.Actogram`` (:958-1000) - with ``cbas_amd.postprocess``.  See INTEGRATION.md.
"""
from __future__ import annotations

import functools
import importlib
import os
import sys


def _workthreads():
    """The reference's ``workthreads`` module, or None where it cannot be imported (it pulls in the GUI's packages)."""
    if "workthreads" in sys.modules:
        return sys.modules["workthreads"]
    try:
        return importlib.import_module("workthreads")
    except Exception:  # noqa: BLE001 - an ImportError of any of its dependencies, or what they raise on import
        return None


def _in_keep_rows(method):
    from .train import keep_rows

    @functools.wraps(method)
    def _execute_training_task(self, *args, **kwargs):
        with keep_rows():
            return method(self, *args, **kwargs)

    _execute_training_task._cbas_amd_wrapped = method
    return _execute_training_task


def _project_path():
    state = sys.modules.get("gui_state")
    return getattr(getattr(state, "proj", None), "path", None)


def _install_postprocess(cbas) -> None:
    """``Dataset.predictions_to_instances*`` and ``Actogram.__init__`` on ``cbas_amd.postprocess``; the originals are kept
    as ``_reference_<name>`` on their classes (a second call keeps the first originals)."""
    from . import postprocess as P

    def predictions_to_instances(self, csv_path, model_name, threshold=0.7):
        video = csv_path.replace(f"_{model_name}_outputs.csv", ".mp4")                      # cbas.py:915
        return P.predictions_to_instances(csv_path, self.config.get("behaviors", []), video, threshold)

    def predictions_to_instances_with_confidence(self, csv_path, model_name, threshold=0.5, smoothing_window=1):
        video = csv_path.replace(f"_{model_name}_outputs.csv", ".mp4")                      # cbas.py:952
        return P.predictions_to_instances_with_confidence(csv_path, self.config.get("behaviors", []), video, threshold,
                                                          smoothing_window, project_path=_project_path())

    def actogram_init(self, behavior, framerate, start, binsize_minutes, threshold, lightcycle, plot_acrophase=False,
                      base_color=None, directory=None, model=None, preloaded_df=None):
        # the attributes Actogram's users read (cbas.py:961-967), the activity through activity_bins, the figure by the
        # reference's own renderer
        self.behavior = behavior
        self.framerate, self.start_hour_on_plot = float(framerate), float(start)
        self.threshold, self.bin_size_minutes = float(threshold), int(binsize_minutes)
        self.plot_acrophase = plot_acrophase
        self.lightcycle_str = {"LL": "1" * 24, "DD": "0" * 24}.get(lightcycle, "1" * 12 + "0" * 12)
        self.blob = None
        self.binned_activity = []
        self.binsize_frames = P.binsize_frames(self.framerate, self.bin_size_minutes)
        if self.binsize_frames <= 0:
            return
        if preloaded_df is not None:
            source = preloaded_df
        elif directory and model:
            source = directory
        else:
            return
        self.binned_activity = P.activity_bins(source, model, None, behavior, self.framerate, self.bin_size_minutes, self.threshold)
        render = getattr(cbas, "_create_matplotlib_actogram", None)
        if not self.binned_activity or render is None:
            return
        fig = render(self.binned_activity, [c == "1" for c in self.lightcycle_str], 24.0, self.bin_size_minutes,
                     f"{model} - {behavior}", self.start_hour_on_plot, self.plot_acrophase, base_color)
        if fig:
            import base64
            import io
            buf = io.BytesIO()
            fig.savefig(buf, format="png", bbox_inches="tight", facecolor="#343a40")
            self.blob = base64.b64encode(buf.getvalue()).decode("utf-8")
            import matplotlib.pyplot as plt
            plt.close(fig)

    for owner, name, new in ((getattr(cbas, "Dataset", None), "predictions_to_instances", predictions_to_instances),
                             (getattr(cbas, "Dataset", None), "predictions_to_instances_with_confidence",
                              predictions_to_instances_with_confidence),
                             (getattr(cbas, "Actogram", None), "__init__", actogram_init)):
        if owner is None:
            continue
        new._cbas_amd_postprocess = True
        old = owner.__dict__.get(name)
        if not getattr(old, "_cbas_amd_postprocess", False):
            setattr(owner, "_reference_" + name, old)
        setattr(owner, name, new)


def _uninstall_postprocess(cbas) -> None:
    for owner, name in ((getattr(cbas, "Dataset", None), "predictions_to_instances"),
                        (getattr(cbas, "Dataset", None), "predictions_to_instances_with_confidence"),
                        (getattr(cbas, "Actogram", None), "__init__")):
        if owner is not None and getattr(owner.__dict__.get(name), "_cbas_amd_postprocess", False):
            old = owner.__dict__.get("_reference_" + name)
            if old is not None:
                setattr(owner, name, old)
            else:
                delattr(owner, name)


def install(strict: bool = True, postprocess: bool = False) -> bool:
    """Returns True when the CBAS modules were found and patched.  ``strict=False`` makes a missing
    CBAS backend a no-op instead of an ImportError.  ``postprocess=True`` also patches ``cbas.Dataset``'s
    ``predictions_to_instances*`` and feeds ``cbas.Actogram`` through ``cbas_amd.postprocess.activity_bins``."""
    try:
        cbas = importlib.import_module("cbas")
        classifier_head = importlib.import_module("classifier_head")
    except ImportError:
        if strict:
            raise
        return False
    from .encoder import DinoEncoder
    from .head import ClassifierLSTMDeltas
    from .pipeline import encode_file, infer_file
    from .train import evaluate_on_split, fit_temperature, train_lstm_model

    cbas._reference_DinoEncoder = getattr(cbas, "DinoEncoder", None)
    cbas._reference_encode_file = getattr(cbas, "encode_file", None)
    cbas._reference_infer_file = getattr(cbas, "infer_file", None)
    cbas._reference_train_lstm_model = getattr(cbas, "train_lstm_model", None)
    if getattr(cbas, "evaluate_on_split", None) is not evaluate_on_split:          # a second install() keeps the original
        cbas._reference_evaluate_on_split = getattr(cbas, "evaluate_on_split", None)
    classifier_head._reference_ClassifierLSTMDeltas = getattr(classifier_head, "ClassifierLSTMDeltas", None)
    cbas.DinoEncoder = DinoEncoder
    cbas.encode_file = encode_file
    cbas.infer_file = infer_file
    cbas.train_lstm_model = train_lstm_model          # TrainingThread, workthreads.py:635
    cbas.evaluate_on_split = evaluate_on_split        # TrainingThread, workthreads.py:675
    classifier_head.ClassifierLSTMDeltas = ClassifierLSTMDeltas
    workthreads = _workthreads()
    if workthreads is not None:
        if getattr(workthreads, "fit_temperature", None) is not fit_temperature:
            workthreads._reference_fit_temperature = getattr(workthreads, "fit_temperature", None)
        workthreads.fit_temperature = fit_temperature  # _save_averaged_training_results, workthreads.py:851
        thread = getattr(workthreads, "TrainingThread", None)
        task = getattr(thread, "_execute_training_task", None)
        if task is not None and not hasattr(task, "_cbas_amd_wrapped"):
            thread._execute_training_task = _in_keep_rows(task)
    if postprocess:
        _install_postprocess(cbas)
    return True


def uninstall() -> None:
    cbas = importlib.import_module("cbas")
    classifier_head = importlib.import_module("classifier_head")
    pairs = [(cbas, ("DinoEncoder", "encode_file", "infer_file", "train_lstm_model", "evaluate_on_split")),
             (classifier_head, ("ClassifierLSTMDeltas",))]
    _uninstall_postprocess(cbas)
    workthreads = _workthreads()
    if workthreads is not None:
        pairs.append((workthreads, ("fit_temperature",)))
        thread = getattr(workthreads, "TrainingThread", None)
        task = getattr(thread, "_execute_training_task", None)
        if hasattr(task, "_cbas_amd_wrapped"):
            thread._execute_training_task = task._cbas_amd_wrapped
    for mod, names in pairs:
        for n in names:
            ref = getattr(mod, "_reference_" + n, None)
            if ref is not None:
                setattr(mod, n, ref)


if os.environ.get("CBAS_USE_MI355X") == "1":  # pragma: no cover
    install(strict=False)
