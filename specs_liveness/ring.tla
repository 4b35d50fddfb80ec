------------------------------ MODULE ring ------------------------------
(* A fair counter cycles modulo N until an unfair process stops it: one component of N states, and nobody has to stop it. *)
EXTENDS Naturals
CONSTANT N
(* --algorithm ring
variables c = 0, stop = 0;

fair process Counter = 0
begin
  C: while stop = 0 do
       c := (c + 1) % N;
     end while;
end process

process Stopper = 1
begin
  S: stop := 1;
end process

end algorithm *)
=============================================================================
