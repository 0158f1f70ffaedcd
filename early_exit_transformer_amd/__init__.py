"""MI355X-native early-exit Conformer encoder (drop-in for the reference's
``models.model.early_exit.Early_conformer`` / ``full_conformer`` encoder path; ``model.Splitformer`` and
``model.Early_zipformer`` are composed from the same kernels)."""
__version__ = "0.1.0"

_CONTEXT = ("ContextGraph", "ContextBiasSession")  # contextual biasing (context.py), resolved at first use: importing the package stays light
_LM_FUSION = ("TokenLM", "LMFusionSession")  # shallow fusion with a token-level n-gram model (lm_fusion.py), likewise
_KEYWORD = ("KeywordSet", "KeywordHits", "keyword_search")  # keyword spotting on CTC emissions (keyword.py), likewise
# word and token timestamps: CTC forced alignment in the standard topology (alignment.py), likewise
_ALIGNMENT = ("Alignment", "TokenSpan", "WordSpan", "ctc_forced_align", "word_spans", "starts_word_from_pieces")
# token posteriors and soft timestamps: CTC forward-backward in the standard topology (posterior.py), likewise
_POSTERIOR = ("Posteriors", "SoftSpan", "SoftWordSpan", "ctc_posteriors", "soft_word_spans", "nbest_posteriors")
# long transcripts: multi-wave CTC segmentation with free ends, utterance spans, windowed emissions (segment.py), likewise
_SEGMENT = ("UtteranceSpan", "ctc_segment", "utterance_spans", "windowed_emission")


def __getattr__(name):
    if name in _SEGMENT:
        from . import segment
        return getattr(segment, name)
    if name in _POSTERIOR:
        from . import posterior
        return getattr(posterior, name)
    if name in _ALIGNMENT:
        from . import alignment
        return getattr(alignment, name)
    if name in _KEYWORD:
        from . import keyword
        return getattr(keyword, name)
    if name in _CONTEXT:
        from . import context
        return getattr(context, name)
    if name in _LM_FUSION:
        from . import lm_fusion
        return getattr(lm_fusion, name)
    raise AttributeError(f"module {__name__!r} has no attribute {name!r}")
