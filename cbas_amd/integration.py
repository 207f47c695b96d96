"""Monkey-patch a running CBAS backend so its unmodified worker threads use the MI355X path.

    import cbas_amd.integration; cbas_amd.integration.install()

Replaces ``cbas.DinoEncoder`` / ``cbas.encode_file`` / ``cbas.infer_file`` (reference
backend/cbas.py:399-572, 650-677) and ``classifier_head.ClassifierLSTMDeltas``
(backend/classifier_head.py:57-172) with the drop-ins of this package, and the training path with it:
``cbas.train_lstm_model``, ``cbas.evaluate_on_split`` (cbas.py:1222-1251) and, when the ``workthreads`` module can be
imported, ``workthreads.fit_temperature`` (workthreads.py:103-137) and ``TrainingThread._execute_training_task``, which
is run inside ``cbas_amd.train.keep_rows()`` so that the runs, trials, test split and calibration of one training job
share one store of CLS rows in device memory.  See INTEGRATION.md.
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


def install(strict: bool = True) -> bool:
    """Returns True when the CBAS modules were found and patched.  ``strict=False`` makes a missing
    CBAS backend a no-op instead of an ImportError."""
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
    return True


def uninstall() -> None:
    cbas = importlib.import_module("cbas")
    classifier_head = importlib.import_module("classifier_head")
    pairs = [(cbas, ("DinoEncoder", "encode_file", "infer_file", "train_lstm_model", "evaluate_on_split")),
             (classifier_head, ("ClassifierLSTMDeltas",))]
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
