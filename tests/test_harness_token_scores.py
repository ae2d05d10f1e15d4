"""--token-scores of the harness (opt-in): the caption / POPE lines gain per-token lists from generate()'s record; without the flag
generate() is called and the lines are written exactly as before.  Stub model, no GPU."""
import json
import types

from dropoutdecoding_amd import harness as H


class _Inputs(dict):
    def to(self, device):
        return self


class _Processor:
    def __init__(self):
        self.tokenizer = types.SimpleNamespace(eos_token_id=2)

    def __call__(self, *a, **k):
        return _Inputs(input_ids=[[1, 5]], pixel_values="px")

    def batch_decode(self, ids, skip_special_tokens=True):
        return [ids]


def _result(text, n):
    rec = {"token_logprobs": [-0.5 * (i + 1) for i in range(n)], "votes": [3 - (i % 2) for i in range(n)],
           "base_token_logprobs": [-0.25 * (i + 1) for i in range(n)]}
    return {"sequences": text, "scores": None, "logits": None, "dropout_record": rec}


class _Model:
    def __init__(self, texts):
        self.texts, self.kw = list(texts), []

    def generate(self, **kw):
        self.kw.append(kw)
        text = self.texts.pop(0)
        return _result(text, 3) if kw.get("return_dict_in_generate") else text


class _Pipeline:
    def __init__(self, texts):
        self.texts, self.kw = list(texts), []

    def run(self, batches, max_new_tokens, eos_token_id=None, **kw):
        self.kw.append(kw)
        for b in batches:
            yield [(_result(self.texts.pop(0), 2) if kw.get("return_dict_in_generate") else self.texts.pop(0)) for _ in b]


TEXTS = ["USER: x ASSISTANT: A cat sits.", "x ASSISTANT: Two dogs."]
ITEMS = [(11, "/img/a.jpg"), (12, "/img/b.jpg")]


def test_flag_parses_and_is_off_by_default():
    base = ["--model-path", "m", "--coco-data-dir", "c"]
    assert H.build_parser().parse_args(base).token_scores is False
    assert H.build_parser().parse_args(base + ["--token-scores"]).token_scores is True


def test_caption_lines_unchanged_without_the_flag(tmp_path):
    model = _Model(TEXTS)
    log = H.CaptionLog(str(tmp_path / "off.json"))
    assert H.caption_images(model, _Processor(), ITEMS, "llava-1.5", log, load_image=lambda p: p, device="cpu") == 2
    assert open(log.path).read() == ('{"image_id": 11, "caption": "A cat sits."}\n{"image_id": 12, "caption": "Two dogs."}\n')
    assert all("return_dict_in_generate" not in kw for kw in model.kw)


def test_caption_lines_gain_the_per_token_lists(tmp_path):
    model = _Model(TEXTS)
    log = H.CaptionLog(str(tmp_path / "on.json"))
    assert H.caption_images(model, _Processor(), ITEMS, "llava-1.5", log, load_image=lambda p: p, device="cpu", token_scores=True) == 2
    assert all(kw["return_dict_in_generate"] is True for kw in model.kw)
    rows = [json.loads(x) for x in open(log.path).read().splitlines()]
    assert rows[0] == {"image_id": 11, "caption": "A cat sits.", "token_logprobs": [-0.5, -1.0, -1.5], "votes": [3, 2, 3],
                       "base_token_logprobs": [-0.25, -0.5, -0.75]}
    assert list(rows[1]) == ["image_id", "caption", "token_logprobs", "votes", "base_token_logprobs"]
    # the reader of the caption log (and its de-duplication) keeps working on such lines
    assert [r["caption"] for r in H.read_caption_log(log.path)] == ["A cat sits.", "Two dogs."]


def test_pipeline_path_passes_the_flag_on(tmp_path):
    pipe = _Pipeline(TEXTS)
    log = H.CaptionLog(str(tmp_path / "p.json"))
    H.caption_images(_Model([]), _Processor(), ITEMS, "llava-1.5", log, load_image=lambda p: p, device="cpu", pipeline=pipe, lanes=2,
                     token_scores=True)
    assert pipe.kw == [{"return_dict_in_generate": True}]
    rows = [json.loads(x) for x in open(log.path).read().splitlines()]
    assert rows[1]["caption"] == "Two dogs." and rows[1]["votes"] == [3, 2] and len(rows[1]["token_logprobs"]) == 2
    pipe2 = _Pipeline(TEXTS)
    log2 = H.CaptionLog(str(tmp_path / "q.json"))
    H.caption_images(_Model([]), _Processor(), ITEMS, "llava-1.5", log2, load_image=lambda p: p, device="cpu", pipeline=pipe2, lanes=2)
    assert pipe2.kw == [{}] and json.loads(open(log2.path).readline()) == {"image_id": 11, "caption": "A cat sits."}


def test_pope_rows_carry_the_answer_tokens_scores(tmp_path):
    qs = [{"image": "a.jpg", "text": "Is there a cat?"}, {"image": "b.jpg", "text": "Is there a car?"}]
    texts = ["USER:  \nIs there a cat? ASSISTANT: Yes", "q ASSISTANT: No"]
    plain = H.answer_pope(_Model(texts), _Processor(), qs, "llava", "/coco", load_image=lambda p: p, device="cpu")
    assert plain == [{"question": "Is there a cat?", "answer": "Yes"}, {"question": "Is there a car?", "answer": "No"}]
    model = _Model(texts)
    rows = H.answer_pope(model, _Processor(), qs, "llava", "/coco", load_image=lambda p: p, device="cpu", token_scores=True)
    assert rows[0] == {"question": "Is there a cat?", "answer": "Yes", "logprob": -0.5, "base_logprob": -0.25}
    assert model.kw[0]["return_dict_in_generate"] is True and model.kw[0]["max_new_tokens"] == 1
    out = tmp_path / "ans.json"
    H.write_pope_answers(str(out), rows)
    assert json.loads(out.read_text().splitlines()[1]) == {"question": "Is there a car?", "answer": "No", "logprob": -0.5, "base_logprob": -0.25}
    H.write_pope_answers(str(out), plain)
    assert json.loads(out.read_text().splitlines()[0]) == {"question": "Is there a cat?", "answer": "Yes"}
