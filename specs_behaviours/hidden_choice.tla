---------------------------- MODULE hidden_choice ----------------------------
(* For mc_engine_behaviours: a hidden choice made at the start.  h is one of K values and is never logged; x is.  Every initial state
   matches the first observation x = 0, so K_0 has K members: with K = 64 (hidden_choice.cfg) the candidate set is exactly full, and
   the step h := h \div 2 folds the members pairwise onto 32 successors — lanes 2j and 2j + 1 of one wavefront bring the same row in the
   same round.  With K = 65 (hidden_choice_65.cfg) K_0 would hold 65 rows: the behaviour is AMBIGUOUS at observation 0. *)
EXTENDS Naturals
CONSTANT K
(* --algorithm hidden_choice
variables h \in 0..K-1, x = 0;

process P = 0
begin
  s: while x < 3 do
       h := h \div 2;
       x := x + 1;
     end while;
end process

end algorithm *)
=============================================================================
