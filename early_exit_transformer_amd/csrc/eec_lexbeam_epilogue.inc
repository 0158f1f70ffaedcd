// The end of both lexicon CTC beam search kernels (ctc_lexbeam.hip, ctc_lexbeam_wide.hip), included as text at the end of the kernel
// body so that each kernel compiles exactly the statements it always had.  It reads the kernel's own names: LM, a, m, bufs, cur, nb, L,
// bp, seq, c, Tq, beam, blank, and the LDS arrays fin_rank, fin_ntok, fin_nw, fin_score (at least max(beam, nbest) entries) and fin_n.
  // the complete hypotheses (node 0) in rank order are best first; one thread walks each one's back-pointers
  if (c == 0) {
    int n = 0;
    if constexpr (LM) {
      // ... after the </s> term they no longer are: ordered by (final score descending, rank ascending), one thread's insertion
      if (L > 0)
        for (int i = 0; i < nb; ++i) {
          const LbBeam e = bufs[cur][i];
          if (e.node != 0) continue;
          float f = e.score;
          if (m.eos >= 0) {
            int next;
            f = lm_add(f, a.lm_weight, lm_walk(m, e.pad, m.eos, next));
          }
          int k = n++;
          for (; k > 0 && f > fin_score[k - 1]; --k) fin_score[k] = fin_score[k - 1], fin_rank[k] = fin_rank[k - 1];
          fin_score[k] = f, fin_rank[k] = i;
        }
      n = min(n, a.nbest);
    } else {
      if (L > 0)
        for (int i = 0; i < nb; ++i)
          if (bufs[cur][i].node == 0 && n < a.nbest) fin_rank[n++] = i;
    }
    fin_n = n;
    a.n_hyp[seq] = n;
  }
  __syncthreads();
  if (c < a.nbest) {
    const size_t o = (size_t)seq * a.nbest + c;
    int n = 0, nw = 0;
    float score = -INFINITY;
    if (c < fin_n) {
      int k = fin_rank[c];
      const LbBeam e = bufs[cur][k];
      n = e.ntok, nw = e.nw, score = LM ? fin_score[c] : e.score;
      int* tok_out = a.tokens + o * Tq;
      int* ts_out = a.timesteps ? a.timesteps + o * Tq : nullptr;
      int* w_out = a.words + o * a.max_words;
      int nt = n, nwd = nw;
      int2 at = bp[(size_t)(L - 1) * beam + k];
      for (int t = L - 1; t >= 0; --t) {
        const int lab = at.x & 0xffff;
        const int2 prev = t > 0 ? bp[(size_t)(t - 1) * beam + (at.x >> 16)] : make_int2(0xffff, 0);
        if (lab != blank && lab != (prev.x & 0xffff) && nt > 0) {  // the first frame of a run of one label
          tok_out[--nt] = lab;
          if (ts_out) ts_out[nt] = t;
        }
        if (at.y && nwd > 0 && --nwd < a.max_words) w_out[nwd] = at.y - 1;
        at = prev;
      }
    }
    a.scores[o] = score;
    a.token_count[o] = n;
    a.word_count[o] = nw;
    fin_ntok[c] = n;
    fin_nw[c] = min(nw, a.max_words);
  }
  __syncthreads();
  // what lies past a hypothesis' counts is -1
  for (int k = c; k < a.nbest * Tq; k += kLbThreads) {
    const int j = k / Tq;
    if (k - j * Tq >= fin_ntok[j]) {
      const size_t o = ((size_t)seq * a.nbest + j) * Tq + (k - j * Tq);
      a.tokens[o] = -1;
      if (a.timesteps) a.timesteps[o] = -1;
    }
  }
  for (int k = c; k < a.nbest * a.max_words; k += kLbThreads) {
    const int j = k / a.max_words;
    if (k - j * a.max_words >= fin_nw[j]) a.words[((size_t)seq * a.nbest + j) * a.max_words + (k - j * a.max_words)] = -1;
  }
