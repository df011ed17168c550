"""`generate_until` with the straggler hand-over under the checkpoint's repetition penalty, through both model plug-ins: the
answers equal those with the hand-over switched off, and `last_timing["handed_over"]` shows that sequences really travelled."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu


# EOS = the most frequent token of these columns of the penalised free run.  Qwen: columns 2:12, as in
# test_generate_until_with_straggler_hand_over_equals_without.  The tiny LLaVA's answers share their first five tokens (one text
# prompt, and its vision tower barely tells the synthetic images apart), so a token of columns 2:6 would end every answer at the same
# step and leave nothing to hand over: columns 6:16.
@pytest.mark.parametrize("model_type,name,size,cols", [("qwen2-vl", "tiny", "56x84", (2, 12)), ("llava", "tiny", "70x120", (6, 16))])
def test_generate_until_hand_over_under_a_penalty_equals_without(gpu, model_type, name, size, cols):
    """90 synthetic documents in engine passes of 24, 24 new tokens, repetition penalty 1.3 on the plug-in's engine, an EOS that many
    answers hit early and some never (the layout of test_generate_until_with_straggler_hand_over_equals_without): the answers - token
    rows and strings - equal those with the hand-over off, and `last_timing["handed_over"]` counts the sequences that travelled
    (observed on MI355X: 25 through the Qwen2-VL plug-in, 20 through the LLaVA one)."""
    from lmms_owc_amd.models import get_model
    from lmms_owc_amd.tasks import load_task

    outs, toks, handed = {}, {}, {}
    for tag in ("carry", "plain"):
        task = load_task(f"synthetic:90:{size}:3")
        task.generation_kwargs.update({"max_new_tokens": 24})
        task.build_all_requests(limit=None, rank=0, world_size=1)
        lm = get_model("custom-model", model_type=model_type, model_name_or_path=f"synthetic:{name}", batch_size=1, engine_batch=24)
        lm._model.repetition_penalty = 1.3
        lm.task_dict[task.task_name] = task.dataset
        if tag == "carry":   # first run: find a token that ends many PENALISED answers early, use it as EOS in both runs
            lm._no_carry = True
            free = lm.generate_until_tokens(task.instances)[0]
            vals, counts = np.unique(free[:, cols[0]:cols[1]], return_counts=True)
            eos = int(vals[np.argmax(counts)])
            lm._no_carry = False
            task.build_all_requests(limit=None, rank=0, world_size=1)
        else:
            lm._no_carry = True
        lm._tokenizer.eos_token_id = eos
        mat, n = lm.generate_until_tokens(task.instances)
        handed[tag] = lm.last_timing["handed_over"]
        assert lm.last_timing["chunks"] >= 3
        toks[tag] = [mat[i, : n[i]].tolist() for i in range(len(n))]
        task.build_all_requests(limit=None, rank=0, world_size=1)
        outs[tag] = lm.generate_until(task.instances)
        assert lm.last_timing["handed_over"] == handed[tag]          # (counted per task, not accumulated)
    print(f"[penalty hand-over] {model_type} plug-in: eos {eos}, {handed['carry']} sequences handed over, "
          f"{len({len(a) for a in toks['carry']})} distinct answer lengths")
    assert toks["carry"] == toks["plain"] and len(toks["carry"]) == 90
    assert outs["carry"] == outs["plain"] and len(outs["carry"]) == 90
    assert len({len(a) for a in toks["carry"]}) > 3      # really ragged
    assert handed["carry"] >= 3 and handed["plain"] == 0, handed
