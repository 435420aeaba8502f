"""Model selection: the reference's nnunetv2/evaluation/find_best_configuration.py:81-211 on volumes in
memory.  Every candidate's cross-validation predictions are scored against the ground truth (evaluation.compute_metrics_on_cases),
every pair of candidates that kept its probabilities is ensembled (ensembling.ensemble_probabilities) and scored, the best
foreground-mean Dice wins, and postprocessing.determine_postprocessing runs on the winner.  Device tensors stay on the device
throughout: K28 averages and counts, K23 labels the components; only confusion matrices are read back."""
import os

from . import ensembling, evaluation, postprocessing


def folds_tuple_to_string(folds):
    """utilities/file_path_utilities.py:78-82"""
    s = str(folds[0])
    for f in folds[1:]:
        s += f"_{f}"
    return s


def get_ensemble_name(model1, model2, folds):
    """utilities/file_path_utilities.py:60-63 (a folder or an identifier trainer__plans__configuration per model)"""
    return "ensemble___" + os.path.basename(model1) + "___" + os.path.basename(model2) + "___" + folds_tuple_to_string(folds)


def _selected(identifier):
    """convert_identifier_to_trainer_plans_config (:15-16) as the return dict's entry; identifiers of another form are kept whole."""
    parts = os.path.basename(identifier).split("__")
    if len(parts) == 3:
        return {"configuration": parts[2], "trainer": parts[0], "plans_identifier": parts[1]}
    return {"identifier": identifier}


def find_best_configuration(candidates, references, foreground_labels, ignore_label=None, allow_ensembling=True,
                            folds=(0, 1, 2, 3, 4)):
    """candidates: an ordered mapping identifier (the reference's trainer__plans__configuration) -> {case_id: (uint8 labels,
    probabilities (K, ...) or None)}; references: {case_id: uint8 labels}; foreground_labels: the labels (or region tuples) to score.
    Every candidate is scored; with allow_ensembling every pair i < j whose members both hold probabilities for all of their cases is
    ensembled (named by get_ensemble_name) and scored.  The largest foreground_mean['Dice'] wins and the first key wins a tie, so a
    single model comes before an ensemble (:142-146).  Returns the reference's return dict: 'folds', 'considered_models',
    'ensembling_allowed', 'all_results' and 'best_model_or_ensemble' with 'result_on_crossval_pre_pp', 'result_on_crossval_post_pp',
    'selected_model_or_models', and 'postprocessing_fns' / 'postprocessing_kwargs' (what postprocessing.apply_postprocessing takes) and
    'postprocessing_summary' in place of the reference's file paths."""
    names = list(candidates)
    if not names:
        raise RuntimeError("find_best_configuration: no candidates")
    labels = list(foreground_labels)
    predictions = {}
    all_results = {}
    for name in names:
        cases = candidates[name]
        if not cases:
            raise RuntimeError(f"find_best_configuration: the candidate {name} has no cases")
        predictions[name] = {c: v[0] for c, v in cases.items()}
        all_results[name] = evaluation.compute_metrics_on_cases(references, predictions[name], labels, ignore_label)["foreground_mean"]["Dice"]
    if allow_ensembling:
        complete = [n for n in names if all(v[1] is not None for v in candidates[n].values())]
        for i, m1 in enumerate(names):
            for m2 in names[i + 1:]:
                if m1 not in complete or m2 not in complete:
                    continue
                if set(candidates[m1]) != set(candidates[m2]):
                    raise RuntimeError(f"the candidates {m1} and {m2} do not hold the same cases")
                name = get_ensemble_name(m1, m2, folds)
                predictions[name] = {c: ensembling.ensemble_probabilities([candidates[m1][c][1], candidates[m2][c][1]])[0]
                                     for c in candidates[m1]}
                all_results[name] = evaluation.compute_metrics_on_cases(references, predictions[name], labels,
                                                                        ignore_label)["foreground_mean"]["Dice"]
    best_score = max(all_results.values())
    best_key = [k for k in all_results if all_results[k] == best_score][0]
    cases = list(predictions[best_key])
    pp_fns, pp_fn_kwargs, summary = postprocessing.determine_postprocessing(
        [predictions[best_key][c] for c in cases], [references[c] for c in cases], labels, ignore_label)
    if best_key.startswith("ensemble___"):
        _, m1, m2, _ = best_key.split("___")
        selected = [_selected(m1), _selected(m2)]
    else:
        selected = [_selected(best_key)]
    return {
        "folds": folds,
        "considered_models": names,
        "ensembling_allowed": allow_ensembling,
        "all_results": all_results,
        "best_model_or_ensemble": {
            "name": best_key,
            "result_on_crossval_pre_pp": all_results[best_key],
            "result_on_crossval_post_pp": summary["postprocessed"]["foreground_mean"]["Dice"],
            "postprocessing_fns": pp_fns,
            "postprocessing_kwargs": pp_fn_kwargs,
            "postprocessing_summary": summary,
            "selected_model_or_models": selected,
        },
    }
