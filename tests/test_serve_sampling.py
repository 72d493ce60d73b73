"""Serving route of top_k / top_p / repeat_penalty requests: on the device
(set_sampling_ex + the graph decode loop) when the engine offers it, the host
loop otherwise.  Offline mock engines, no GPU."""
import numpy as np
import pytest

from cake_amd.serve import GenSession, apply_repeat_penalty, create_app
from tests.test_serve import MockEngine


class CountingEngine(MockEngine):
    def __init__(self):
        super().__init__()
        self.prefills = 0
        self.decodes = 0
        self.logit_prefills = 0
        self.calls = []

    def prefill(self, ids, want_logits=False):
        self.prefills += 1
        self.logit_prefills += int(want_logits)
        return super().prefill(ids, want_logits)

    def decode(self, n):
        self.decodes += 1
        return super().decode(n)

    def set_sampling(self, temperature, seed=299792458):
        self.calls.append(("set_sampling", temperature, seed))


class ExEngine(CountingEngine):
    def set_sampling_ex(self, temperature, top_k=0, top_p=1.0,
                        repeat_penalty=1.0, repeat_last_n=128,
                        seed=299792458):
        self.calls.append(("set_sampling_ex", temperature, top_k, top_p,
                           repeat_penalty, repeat_last_n, seed))


def _post(engine, body):
    from fastapi.testclient import TestClient
    r = TestClient(create_app(engine, model_name="mock")).post(
        "/v1/chat/completions", json=body)
    assert r.status_code == 200
    return r.json()["choices"][0]["token_ids"]


def test_top_p_and_penalty_run_on_the_device_when_offered():
    eng = ExEngine()
    toks = _post(eng, {"prompt_token_ids": [1, 2, 3], "max_tokens": 20,
                       "temperature": 0.8, "top_p": 0.95,
                       "repeat_penalty": 1.1, "seed": 4})
    assert toks == list(range(4, 24))
    assert eng.calls == [("set_sampling_ex", 0.8, 0, 0.95, 1.1, 128, 4)]
    # served by the decode loop: one prompt prefill, no per-token logits
    assert eng.prefills == 1 and eng.logit_prefills == 0
    assert eng.decodes >= 1


def test_penalty_alone_and_top_k_alone_take_the_device_route():
    eng = ExEngine()
    _post(eng, {"prompt_token_ids": [7], "max_tokens": 4,
                "repeat_penalty": 1.2, "repeat_last_n": 64})
    _post(eng, {"prompt_token_ids": [7], "max_tokens": 4,
                "temperature": 1.0, "top_k": 40})
    assert eng.calls == [
        ("set_sampling_ex", 0.0, 0, 1.0, 1.2, 64, 299792458),
        ("set_sampling_ex", 1.0, 40, 1.0, 1.0, 128, 299792458)]
    assert eng.logit_prefills == 0


def test_plain_requests_keep_set_sampling():
    eng = ExEngine()
    _post(eng, {"prompt_token_ids": [7], "max_tokens": 4,
                "temperature": 0.7, "seed": 9})
    _post(eng, {"prompt_token_ids": [7], "max_tokens": 4,
                "temperature": 0.7, "top_p": 1.0, "repeat_penalty": 1.0})
    assert [c[0] for c in eng.calls] == ["set_sampling", "set_sampling"]


def test_engine_without_the_setter_takes_the_host_loop():
    eng = CountingEngine()
    toks = _post(eng, {"prompt_token_ids": [1, 2, 3], "max_tokens": 5,
                       "temperature": 0.8, "top_p": 0.95})
    assert len(toks) == 5
    assert eng.logit_prefills == 5 and eng.decodes == 0
    assert eng.calls == []
    plain = MockEngine()
    assert len(_post(plain, {"prompt_token_ids": [1], "max_tokens": 3,
                             "temperature": 0.8, "top_k": 2})) == 3


def test_host_fallback_honours_the_penalty():
    """MockEngine's logits peak at last+1 (10), last+2 (9), last+3 (8) and
    are 0 elsewhere; greedy with a strong penalty must avoid what it has
    already produced, without one it follows the peak."""
    plain = list(GenSession(MockEngine()).generate_sampled(
        [5], 4, temperature=0.0, top_k=None, top_p=None, seed=1))
    assert plain == [6, 7, 8, 9]
    s = GenSession(MockEngine())
    got = list(s.generate_sampled([5], 3, temperature=0.0, top_k=None,
                                  top_p=None, seed=1, repeat_penalty=1.3,
                                  repeat_last_n=8))
    assert got[:2] == [6, 7]
    x = np.array([2.0, -2.0, 0.0, 5.0], dtype=np.float32)
    out = apply_repeat_penalty(x, 2.0, [0, 1, 2, 0])
    assert list(out) == [1.0, -4.0, 0.0, 5.0]
    assert list(x) == [2.0, -2.0, 0.0, 5.0]


def test_penalty_request_on_plain_mock_is_served():
    toks = _post(MockEngine(), {"prompt_token_ids": [5], "max_tokens": 4,
                                "repeat_penalty": 1.3})
    assert len(toks) == 4
