------------------------------ MODULE two_loops ------------------------------
(* Two cycles with steps from the first into the second.  While phase = 0 the counter runs modulo 4 and the fair process Fin waits: a fair cycle that never terminates.  Once the unfair Switch has set phase, the counter runs modulo 2 and Fin is enabled all the time: weak fairness takes it out of that cycle.  The first cycle holds the later states, so its colour reaches the second. *)
EXTENDS Naturals

(* --algorithm two_loops
variables a = 0, phase = 0, go = 1;

process Toggler = 0
begin
  T: while go = 1 do
       a := IF phase = 0 THEN (a + 1) % 4 ELSE (a + 1) % 2;
     end while;
end process

process Switch = 1
begin
  S: phase := 1;
end process

fair process Fin = 2
begin
  F:  await phase = 1;
  F2: go := 0;
end process

end algorithm *)
=============================================================================
