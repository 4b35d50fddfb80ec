----------------------------- MODULE hidden_late -----------------------------
(* For mc_engine_behaviours: a hidden choice made on every step.  One initial state; each step picks h among K values and counts x up.
   Logging x alone, K_0 has one member and K_1 has K: with K = 65 (hidden_late_65.cfg) the behaviour is AMBIGUOUS at observation 1,
   not 0 — one lane brings 65 successors, one per round.  With K = 64 (hidden_late.cfg) K_1 is full and, at observation 2, each of 64
   lanes brings the same 64 rows: the set stays at 64. *)
EXTENDS Naturals
CONSTANT K
(* --algorithm hidden_late
variables h = 0, x = 0;

process P = 0
begin
  s: while x < 3 do
       with v \in 0..K-1 do
         h := v;
       end with;
       x := x + 1;
     end while;
end process

end algorithm *)
=============================================================================
